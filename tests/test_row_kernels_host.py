"""The comparators of tests/row_kernel_cases.py are attainable and discriminating, shown on the CPU before a GPU is involved: a numpy-float32 restatement of every
kernel form (scalar, four-column with the REM = 128 tail, eight-column summation orders; the fp8 row quantisation; the three softmaxes) passes every case that
tests/test_gpu_row_kernels.py runs, and each mutant -- the slips that the whole-network tolerances of 3e-2 / 2.56e-2 let through -- fails a case named here."""
import numpy as np
import pytest

import row_kernel_cases as R


def _forms(D):
    """every kernel form that exists for D (the launcher picks one of them; the others are restated all the same)"""
    return [0] + ([1] if D in R.LN_D_VECTOR else []) + ([2] if D % 512 == 0 else [])


def _run_ln(c, form, fp8, mutant=None, qmutant=None):
    v, n = R.ln_restated(c, form, fp8, mutant)
    if not fp8:
        return R.check_bf16(c, R.f32_to_bf16_bits(v))
    q, s = R.quant_restated(v, qmutant, amax_from=n if qmutant == "amax_before_modulation" else None)
    return R.check_fp8(c["y"], c["delta"], q, s, exact=R.exact_rows(c))


def _rows_of(c, *families):
    return {i for i, f in enumerate(c["families"]) if f in families}


def test_number_format_helpers():
    t = R.E4M3
    assert t[0x7e] == 448.0 and t[0xfe] == -448.0 and np.isnan(t[0x7f]) and np.isnan(t[0xff]) and t[0x01] == 2.0 ** -9 and t[0x08] == 2.0 ** -6 and t[0x38] == 1.0
    assert np.all(np.diff(t[:0x7f]) > 0)
    good = [b for b in range(256) if b & 0x7f != 0x7f]
    assert np.array_equal(R.f32_to_e4m3(t[good].astype(np.float32)), np.array(good, np.uint8))            # encode(decode(b)) = b
    assert R.f32_to_e4m3(np.float32([17.0, 19.0, 17.0001, -1e-9, 500.0, -500.0])).tolist() == [0x58, 0x5a, 0x59, 0x80, 0x7e, 0xfe]      # ties to even; the clamp
    assert R.f32_to_e4m3(np.float32([17.9]), truncate=True).tolist() == [0x58] and R.f32_to_e4m3(np.float32([448.01]), saturate_first=False).tolist() == [0x7f]
    assert R.e4m3_ulp(np.array([0.0, 2.0 ** -7, 2.0 ** -6, 1.0, 1.99, 448.0, 1e6])).tolist() == [2.0 ** -9, 2.0 ** -9, 2.0 ** -9, 0.125, 0.125, 32.0, 32.0]
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -30), 2.0 ** -133 * 1.5, 3.39e38, 3.4e38])
    assert R.rne_bf16(v).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), 2.0 ** -132, 2.0 ** 127 * (2 - 2.0 ** -7), np.inf]
    r = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 7
    assert np.array_equal(R.bf16_bits_to_f64(R.f32_to_bf16_bits(r)), R.rne_bf16(r.astype(np.float64)))   # the two roundings agree


def test_ln_cases_reach_every_path():
    assert (R.B, R.RPS, R.ROWS) == (3, 5, 15) and set(R.FAMILIES) == {1, 2, 3, 4, 5, 6, 7}
    assert len(R.ln_case_ids(False)) == 2 * (9 + 4) and len(R.ln_case_ids(True)) == 2 * (9 + 3)        # D = 64 is bf16 only
    for D, half, lay in R.ln_case_ids(False):
        c = R.ln_case(D, half, lay)
        assert c["x"].dtype == (np.float16 if half else np.float32) and c["mod_ld"] == 6 * D + (lay == "odd_mod_ld")
        assert c["form"] == (0 if lay != "aligned" or D not in (256, 1152, 1536) else 2 if half and D == 1536 else 1)
        aligned = c["mod_ld"] % 4 == 0 and c["shift_off"] % 4 == 0 and c["scale_off"] % 4 == 0
        assert aligned == (lay == "aligned")
        assert np.all(c["shift"][2] == 0) and np.all(c["shift"][:2] != 0) and c["x"][4, D - 3] == 1e4 and np.all(c["x"][10] == 0.5)
        assert np.isnan(c["mod"]).sum() == c["mod"].size - 2 * R.B * D                                     # everything but shift and scale is NaN
        if half:
            h = np.abs(c["x"][R.HALF_EXTRA_ROW].astype(np.float64))
            assert c["families"][R.HALF_EXTRA_ROW] == "H" and (h == 60000).any() and ((h > 0) & (h < 2.0 ** -14)).any() and np.isfinite(c["y"]).all()


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_restated_ln_forms_pass(fp8):
    """every form that exists for a case's D, not only the one the launcher picks; the raw fp32 error of the restatement stays within a quarter of the radius"""
    worst, raw = 0.0, 0.0
    for D, half, lay in R.ln_case_ids(fp8):
        c = R.ln_case(D, half, lay)
        for form in _forms(D):
            bad, ratio = _run_ln(c, form, fp8)
            assert not bad, (c["name"], form, bad)
            worst = max(worst, ratio)
            v, _ = R.ln_restated(c, form, fp8)
            raw = max(raw, float(np.max(np.abs(v.astype(np.float64) - c["y"])[c["delta"] > 0] / c["delta"][c["delta"] > 0])))
    print(f"\nrestated LayerNorm-modulate, {'fp8' if fp8 else 'bf16'}: worst |fp32 value - y| / delta = {raw:.3f}; worst comparator figure = {worst:.3f}")
    assert raw <= 0.25


# mutant -> the case (D, half stream, layout), the form restated, and the row families that must fail there
LN_MUTANT_CASES = {
    "eps_1e-5": ((256, False, "aligned"), 1, (3,)),                     # family 3: the epsilon decides the result
    "var_over_D-1": ((1536, True, "aligned"), 2, (1, 6)),              # 3e-4 relative at the widest D: a seventh of a bf16 half-ulp, over 1536 columns
    "stats_without_tail": ((1152, False, "aligned"), 1, (1, 5)),       # family 5: the 1e4 of column D - 3 sits in the tail
    "tail_rotated_by_4": ((1152, True, "aligned"), 1, (1, 3, 5, 6, "H")),      # (family 2 as fp16 is a few distinct values: one such row survives)
    "shift_scale_swapped": ((384, False, "aligned"), 0, (1, 2, 3, 4, 5, 6)),
}


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("mutant", list(LN_MUTANT_CASES))
def test_ln_mutants_fail(mutant, fp8):
    cid, form, families = LN_MUTANT_CASES[mutant]
    c = R.ln_case(*cid)
    bad, _ = _run_ln(c, form, fp8, mutant)
    assert _rows_of(c, *families) <= set(bad), (mutant, bad)
    assert not _run_ln(c, form, fp8)[0]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("cid", [(1536, False, "aligned"), (256, True, "moved_one_float")], ids=["four-column", "scalar"])
def test_sample_index_off_by_one_fails_at_the_sample_boundaries_only(cid, fp8):
    c = R.ln_case(*cid)
    assert _run_ln(c, c["form"], fp8, "sample_index_row+1")[0] == [4, 9, 14]       # the last row of each sample, nothing else


FP8_CASE = (1152, False, "aligned")


def test_fp8_mutants_fail():
    c = R.ln_case(*FP8_CASE)
    live = _rows_of(c, 1, 2, 3, 5, 6)
    bad, _ = _run_ln(c, 1, True, qmutant="e4m3_truncated")
    assert live <= set(bad)
    bad, _ = _run_ln(c, 1, True, qmutant="amax_before_modulation")
    assert live <= set(bad)
    # no clamp: under the pessimistic model of a non-saturating convert (R.f32_to_e4m3) the largest element encodes NaN in the rows whose fp32 product
    # amax * (1 / (amax / 448)) lands above 448 -- about a third of them; the rows that fail are exactly those
    c = R.ln_case(256, False, "aligned")
    v, _ = R.ln_restated(c, 1, True)
    amax = np.abs(v).max(axis=1)
    qs = np.where(amax > 0, amax / np.float32(448), np.float32(1)).astype(np.float32)
    over = set(np.nonzero((amax * (np.float32(1) / qs)).astype(np.float32) > 448)[0].tolist())
    bad, _ = _run_ln(c, 1, True, qmutant="no_clamp")
    assert over and set(bad) == over, (bad, over)


def test_restated_pack_passes_and_its_mutants_fail():
    hit = {"e4m3_truncated": [], "no_clamp": []}
    for K, kinds in R.pack_cases():
        w = R.pack_case(K, kinds)
        assert w.shape == (len(kinds), K) and all((w[i] == 0).all() for i, k in enumerate(kinds) if k == "zero")
        assert all(w[i, np.abs(w[i]).argmax()] < 0 for i, k in enumerate(kinds) if k == "negative_max")
        q, s = R.quant_restated(w)
        assert not R.check_fp8(w, None, q, s)[0], (K, kinds)
        for m in hit:
            q, s = R.quant_restated(w, m)
            if R.check_fp8(w, None, q, s)[0]:
                hit[m].append((K, len(kinds)))
    assert (1152, 1) in hit["e4m3_truncated"] and (1152, 5) in hit["e4m3_truncated"], hit
    assert hit["no_clamp"], hit


def test_restated_softmaxes_pass_and_their_mutants_fail():
    worst = 0.0
    for kind, T, fams in R.softmax_cases():
        s = R.softmax_rows(T, fams)
        bad, ratio = R.check_softmax(s, fams, R.softmax_restated(s, kind))
        assert not bad, (kind, T, fams, bad)
        worst = max(worst, ratio)
    print(f"\nrestated softmaxes: worst (|bf16 - p| - half ulp) / (eps p) = {worst:.3f}")
    assert [len(R.SOFTMAX_T[k]) for k in (0, 1, 2)] == [4, 3, 3] and len(R.softmax_cases()) == 10 * 8
    fams = R.SOFTMAX_FAMILIES
    # without the max subtraction exp overflows where N(0, 30) exceeds 88.7: inf / inf in that row (T = 576: the kind-1 case), nothing to see at T <= 256
    s = R.softmax_rows(576, fams)
    assert R.check_softmax(s, fams, R.softmax_restated(s, 1, "no_max_subtraction"))[0] == [fams.index("normal_x30")]
    # normalised by T: right only where every entry is equal
    s = R.softmax_rows(100, fams)
    assert R.check_softmax(s, fams, R.softmax_restated(s, 0, "normalised_by_T"))[0] == [i for i, f in enumerate(fams) if f != "all_equal"]
