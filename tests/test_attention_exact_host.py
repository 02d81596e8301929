"""tests/attention_exact_cases.py on the host: the conditions that make its expected bytes exact, an fp64 softmax of the small cases, and the checker's
sensitivity -- four deliberately wrong attention outputs computed on the CPU must be rejected (no kernel is touched here)."""
import math

import numpy as np
import pytest

import attention_exact_cases as X

MMDIT_T = (64, 65, 129, 285, 1100, 4429)
DIT_T = (256, 384, 1024)


def test_one_over_T_has_one_byte_whatever_the_form():
    t = np.arange(1, 4500, dtype=np.float32)
    one = np.float32(1.0)
    a = X.bf16_bits(one / t)                                              # fp32 division
    b = X.bf16_bits((1.0 / t.astype(np.float64)).astype(np.float32))      # the fp64 quotient
    c = X.bf16_bits(one * (one / t))                                      # reciprocal, then multiply
    assert np.array_equal(a, b) and np.array_equal(a, c)
    for T in MMDIT_T + DIT_T:
        bits = X.check_one_over_T(T)                                      # (asserts the 7.8e-4 distance from a rounding boundary)
        assert abs(float(X.bf16_f32(np.uint16(bits))) * T - 1.0) <= 2.0 ** -8


def test_bf16_helpers_round_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e-3, 2.0 ** 15, 0.0], np.float32)       # 1 + 2^-8 ties to even (1.0); 1 + 3 * 2^-8 ties to 1 + 2^-6
    bits = X.bf16_bits(x)
    assert bits.tolist()[:3] == [0x3F80, 0x3F80, 0x3F82] and bits[4] == 0x4700 and bits[5] == 0
    assert np.array_equal(X.bf16_bits(X.bf16_f32(bits)), bits)


@pytest.mark.parametrize("T,hd,A", [(4429, 64, 16), (1024, 72, 16), (1024, 96, 16), (256, 8, None), (1024, 16, 32), (1024, 40, 16), (1024, 56, 16), (384, 64, 16), (1024, 80, 16), (1024, 88, 16)])
def test_selector_conditions(T, hd, A):
    """the gap, the exponent bound and the leak bound are asserted by the builder; here: the multipliers A at the four corner shapes and at every other head width"""
    c = X.selector_case(2, 2, T, hd, seed=T + hd)
    i = c.info
    assert i["gap"] >= X.MIN_GAP_NATS and i["A"] * math.sqrt(hd) * X.LOG2E < X.MAX_EXPONENT
    assert i["leak"] < 2.0 ** -19 * X.V_FLOOR                              # half a bf16 ulp of the smallest value is 2^-9 of it
    if A is not None:
        assert i["A"] == A
    else:
        # all 256 words of length 8: the nearest neighbours differ in one position (ip = 6).  The power of two with the gap, 64, breaks the exponent bound
        # (64 * 8^0.5 * log2 e = 261), so the builder takes the smallest integer with the gap
        assert i["max_off"] == 6 and i["A"] == 57
    q = X.bf16_f32(c.q)
    assert set(np.unique(np.abs(q)).tolist()) == {float(i["A"])}           # exact in bf16
    for (b, h), p in i["perms"].items():
        assert sorted(p.tolist()) == list(range(T)) and not (p == np.arange(T)).any()
        ntiles = -(-T // 64)
        for edge in range(64, T, 64):                                       # queries on each side of every 64-key tile boundary select keys on the other side ...
            assert (p[:edge] >= edge).any() and (p[edge:] < edge).any()
            assert len(np.unique(p[edge - 64:edge] // 64)) >= min(ntiles, 8)       # ... and the 64 queries of a tile select from many key tiles


def test_selector_needs_enough_code_words():
    with pytest.raises(AssertionError, match="2\\^hd"):
        X.selector_case(1, 1, 384, 8)


def test_uniform_case_ownership():
    c = X.uniform_case(2, 3, 285, 64, seed=1)
    v = X.bf16_f32(c.v)
    assert v.sum() == 285 and (v.reshape(2, 285, -1).sum(axis=(0, 2)) == 1).all()       # every key owns exactly one column
    assert (X.bf16_f32(c.q) == 0).all() and (c.expect == 0).sum() == 2 * 285 * 64 * 3 - 285 * 285
    with pytest.raises(AssertionError, match="own a column"):
        X.uniform_case(1, 1, 65, 64)


@pytest.mark.parametrize("engine_layout", [False, True])
@pytest.mark.parametrize("T", [65, 129, 285])
@pytest.mark.parametrize("family", ["uniform", "selector"])
def test_fp64_softmax_rounds_to_the_expected_bytes_mmdit(family, T, engine_layout):
    c = (X.uniform_case(2, 3, T, 64, seed=T) if family == "uniform" else X.selector_case(2, 2, T, 64, seed=T))
    p = X.pack_mmdit(c, engine_layout=engine_layout)
    X.check_output(c, X.reference_mmdit(p))
    if family == "selector":                                               # NaN in the padded key rows: ignored by a softmax over the keys < T
        X.check_output(c, X.reference_mmdit(X.pack_mmdit(c, engine_layout=engine_layout, k_pad=float("nan"))))


@pytest.mark.parametrize("gapped", [False, True])
@pytest.mark.parametrize("hd", [8, 40, 96])
@pytest.mark.parametrize("family", ["uniform", "selector"])
def test_fp64_softmax_rounds_to_the_expected_bytes_dit(family, hd, gapped):
    T = 256
    H = max(2, -(-T // (2 * hd)))
    c = X.uniform_case(2, H, T, hd, seed=hd) if family == "uniform" else X.selector_case(2, 2, T, hd, seed=hd)
    X.check_output(c, X.reference_dit(X.pack_dit(c, gapped=gapped)))


@pytest.mark.parametrize("engine_layout", [False, True])
@pytest.mark.parametrize("bug", X.BUGS)
def test_checker_rejects_wrong_outputs(bug, engine_layout):
    """one valid key dropped, one padded key admitted, two heads exchanged, the sequence stride off by one row: each computed in fp64 on the CPU from the packed
    operands.  Every mistake must be caught by the family that is built to see it (a padded key scores 40 nats below the selected one, so only the uniform family
    -- or NaN padding -- sees it; with q = 0 and every row alike, a query-side stride slip is the selector family's to see), most by both."""
    T = 285
    cases = {"uniform": X.uniform_case(2, 3, T, 64, seed=3), "selector": X.selector_case(2, 2, T, 64, seed=3)}
    seen = {}
    for name, c in cases.items():
        p = X.pack_mmdit(c, engine_layout=engine_layout)
        X.check_output(c, X.reference_mmdit(p))                            # the same code without the mistake passes
        try:
            X.check_output(c, X.reference_mmdit(p, bug=bug))
            seen[name] = False
        except AssertionError:
            seen[name] = True
    want = {"drop_key": ("uniform", "selector"), "admit_pad": ("uniform",), "swap_heads": ("uniform", "selector"), "seq_stride": ("selector",)}[bug]
    assert all(seen[f] for f in want), (bug, seen)
    if bug == "admit_pad":                                                  # the selector family sees it through NaN padding
        c = cases["selector"]
        with pytest.raises(AssertionError, match="differ"):
            X.check_output(c, X.reference_mmdit(X.pack_mmdit(c, engine_layout=engine_layout, k_pad=float("nan")), bug=bug))


def test_checker_rejects_a_touched_canary_and_a_single_bit():
    c = X.selector_case(2, 2, 129, 64, seed=5)
    p = X.pack_mmdit(c, engine_layout=True)
    good = X.reference_mmdit(p)
    X.check_output(c, good)
    for where in ((1, 7, p["D"] + 3), (0, p["Tp"] + 1, 5)):                # a gap column, a gap row
        o = good.copy(); o[where] = 0
        with pytest.raises(AssertionError, match="overwritten"):
            X.check_output(c, o)
    o = good.copy(); o[1, 128, 100] ^= 1                                    # the last bit of one element of the last valid row
    with pytest.raises(AssertionError, match="row 128 head 1 channel 36"):
        X.check_output(c, o)
    o = good.copy(); o[0, 129:256, :p["D"]] = 0x1234                        # rows T .. Tp-1 are unspecified
    X.check_output(c, o)


def test_mx_exact_blocks_and_scale_bytes():
    vals, codes, sc = X.mx_exact_values(2, 129, 4, seed=1)
    blk = np.abs(vals).reshape(2, 129, 4, 2, 32)
    amax = blk.max(axis=-1)
    assert np.array_equal(X.mx_scale_byte(amax), sc.astype(np.int64)) and sc.min() >= 121 and sc.max() <= 133
    mant = amax / np.exp2(np.floor(np.log2(amax)))
    assert (mant > 1.0).all() and (mant < 1.75).all() and (blk > 0).all()
    assert (np.sort(blk, axis=-1)[..., -2] < amax * (256.0 / 288.0) + 1e-12).all()      # the maximum is alone in its binade
    scaled = vals.reshape(2, 129, 4, 2, 32) / np.exp2(sc.astype(np.float32) - 127)[..., None]
    assert np.array_equal(X.e4m3_value(codes).reshape(scaled.shape), scaled) and np.abs(scaled).max() <= 416
    torch = pytest.importorskip("torch")
    if hasattr(torch, "float8_e4m3fn"):                                     # the byte decoder against torch's
        allb = np.arange(256, dtype=np.uint8)
        ref = torch.from_numpy(allb).view(torch.float8_e4m3fn).float().numpy()
        ok = ~np.isnan(ref)
        assert np.array_equal(X.e4m3_value(allb)[ok], ref[ok])
    assert X.mx_scale_byte(np.array([448.0, 448.5, 224.0, 0.0, 1.0])).tolist() == [127, 128, 126, 127, 119]
    assert X.omx_index(1, 3, 5, 1, H=4, Tp=256) == 256 * 8 + (256 + 5) * 4 + 3
