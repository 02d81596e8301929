"""The row kernels of the transformer and VAE paths ALONE against fp64 (tests/row_kernel_cases.py: cases, references, radii and comparators; their attainability
and the mutants they catch: tests/test_row_kernels_host.py): LayerNorm-modulate to bf16 and to fp8 through natinf_debug_ln_modulate -- the engines' launchers, with the
kernel form they pick asserted per case --, k_pack_fp8_rows through natinf_debug_quant_fp8_rows, and the three row softmaxes through natinf_debug_softmax_rows.
Every output sits between canaries that must come back untouched; no case and no element is left out of a comparison.

Worst figures measured on an MI355X (each test prints its own; a figure of 1 would be the edge of the radius; the part of an error that hides inside the output
format's own rounding, half a bf16 / e4m3 ulp, is not counted, so 0.000 means `below the output's rounding`):
  LayerNorm-modulate, bf16 and fp8 alike: scalar form 0.059 (D 1408, fp32 stream), four-column 0.021 (D 1536, fp32 stream), eight-column 0.013 (D 1536, half stream);
  k_pack_fp8_rows: |decode - w / s| / half an e4m3 ulp = 1.000 at the worst (never beyond);
  softmax: k_softmax_rows 0.000, k_softmax_rows_1k 0.024 (T 1024, N(0, 1)), k_softmax_rows_wide 0.000.
All 142 cases pass: no defect found, no kernel changed."""
import numpy as np
import pytest
import torch

import row_kernel_cases as R

pytestmark = pytest.mark.gpu

BF16_CANARY = 0x7fc0


def _dev(a):
    a = np.array(a, order="C")                                          # a copy: the cases are shared and read-only
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.float16): np.float16}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(view)).cuda()


def _run_ln(c, fp8):
    """one natinf_debug_ln_modulate call on the case's operands; returns (form, bf16 bits | (bytes, scales)) after checking the canaries"""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    import ctypes as C
    D, rows = c["D"], R.ROWS
    x, mod = _dev(c["x"]), _dev(c["mod"])
    shift, scale = ptr(mod) + 4 * c["shift_off"], ptr(mod) + 4 * c["scale_off"]
    form = C.c_int(-1)
    if not fp8:
        h = torch.full((rows + 2, D), BF16_CANARY, dtype=torch.int16, device="cuda")      # one canary row before and one after
        check(lib.natinf_debug_ln_modulate(ptr(x), int(c["half"]), shift, scale, c["mod_ld"], ptr(h) + 2 * D, None, None, D, rows, R.RPS, C.byref(form), stream_ptr()),
              "natinf_debug_ln_modulate")
        torch.cuda.synchronize()
        out = h.cpu().numpy().view(np.uint16)
        assert np.all(out[0] == BF16_CANARY) and np.all(out[-1] == BF16_CANARY), "a canary row around h was written"
        return form.value, out[1:-1]
    q = torch.full((rows + 2, D), 0x7f, dtype=torch.uint8, device="cuda")
    s = torch.full((rows + 2,), float("nan"), dtype=torch.float32, device="cuda")        # (rows + 1 would do: the element before row_scale[0] is a canary too)
    check(lib.natinf_debug_ln_modulate(ptr(x), int(c["half"]), shift, scale, c["mod_ld"], None, ptr(q) + D, ptr(s) + 4, D, rows, R.RPS, C.byref(form), stream_ptr()),
          "natinf_debug_ln_modulate")
    torch.cuda.synchronize()
    qh, sh = q.cpu().numpy(), s.cpu().numpy()
    assert np.all(qh[0] == 0x7f) and np.all(qh[-1] == 0x7f), "a canary around the fp8 plane was written"
    assert np.isnan(sh[0]) and np.isnan(sh[-1]), "the canary after row_scale[rows - 1] (or before row_scale[0]) was written"
    return form.value, (qh[1:-1], sh[1:-1])


@pytest.mark.parametrize("D,half,layout", R.ln_case_ids(False), ids=lambda v: str(v))
def test_ln_modulate_bf16(D, half, layout):
    """k_ln_modulate / k_ln_modulate_v4<1,0 | 4,128 | 6,0, false | true> / k_ln_modulate_h8<3> with RowsBf16 (csrc/transformer_rows.h): every element within [rne_bf16(y - delta), rne_bf16(y + delta)], the constant
    rows equal to bf16(shift), the form the launcher chose as tests/row_kernel_cases.py::expected_form states it"""
    c = R.ln_case(D, half, layout)
    form, bits = _run_ln(c, False)
    bad, ratio = R.check_bf16(c, bits)
    print(f"\nln_modulate bf16 {c['name']}: form {form}, worst (|h - y| - half ulp) / delta = {ratio:.3f}")
    assert form == c["form"]
    assert not bad, f"rows {bad} (families {[c['families'][i] for i in bad]}) outside the radius"


@pytest.mark.parametrize("D,half,layout", R.ln_case_ids(True), ids=lambda v: str(v))
def test_ln_modulate_fp8(D, half, layout):
    """The same kernels with RowsFp8: R.check_fp8 -- the row scale, half an e4m3 ulp per byte, no NaN byte, the row maximum
    at +-448, the all-zero rows (scale 1.0, bytes 0), the constant rows the quantised shift with no radius at all"""
    c = R.ln_case(D, half, layout)
    form, (q, s) = _run_ln(c, True)
    bad, ratio = R.check_fp8(c["y"], c["delta"], q, s, exact=R.exact_rows(c))
    print(f"\nln_modulate fp8 {c['name']}: form {form}, worst (|decode - y / s| - half ulp) / (delta / s) = {ratio:.3f}")
    assert form == c["form"]
    assert not bad, f"rows {bad} (families {[c['families'][i] for i in bad]}) fail the fp8 comparator"


@pytest.mark.parametrize("K,kinds", R.pack_cases(), ids=lambda v: str(v) if isinstance(v, int) else "+".join(v))
def test_pack_fp8_rows(K, kinds):
    """k_pack_fp8_rows: the same comparator with delta = 0 and the scale equal to float32(amax) / 448 up to 2u"""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    w = R.pack_case(K, kinds)
    rows, pad = len(kinds), 16                                          # canary bytes before and after the plane (the kernel stores byte pairs)
    q = torch.full((pad + rows * K + pad,), 0x7f, dtype=torch.uint8, device="cuda")
    s = torch.full((rows + 2,), float("nan"), dtype=torch.float32, device="cuda")
    wd = _dev(w)
    check(lib.natinf_debug_quant_fp8_rows(ptr(wd), ptr(q) + pad, ptr(s) + 4, rows, K, stream_ptr()), "natinf_debug_quant_fp8_rows")
    torch.cuda.synchronize()
    qh, sh = q.cpu().numpy(), s.cpu().numpy()
    assert np.all(qh[:pad] == 0x7f) and np.all(qh[-pad:] == 0x7f) and np.isnan(sh[0]) and np.isnan(sh[-1]), "a canary was written"
    qr, sr = qh[pad:-pad].reshape(rows, K), sh[1:-1]
    bad, _ = R.check_fp8(w, None, qr, sr)
    live = [i for i, k in enumerate(kinds) if k != "zero"]
    t = w[live].astype(np.float64) / sr[live].astype(np.float64)[:, None]
    worst = float(np.max(np.abs(R.E4M3[qr[live]] - t) / (0.5 * R.e4m3_ulp(t)))) if live else 0.0
    print(f"\npack_fp8_rows K {K} {kinds}: worst |decode - w / s| / half ulp = {worst:.3f}")
    assert not bad, f"rows {bad} fail the fp8 comparator"


@pytest.mark.parametrize("kind,T,families", R.softmax_cases(), ids=lambda v: str(v) if isinstance(v, int) else ("7rows" if len(v) > 1 else v[0]))
def test_softmax_rows(kind, T, families):
    """k_softmax_rows / k_softmax_rows_1k / k_softmax_rows_wide: [rne_bf16(p (1 - eps) - 2^-126), rne_bf16(p (1 + eps) + 2^-126)] per element; 1 / T exactly in an
    all-equal row of a power-of-two T"""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    s = R.softmax_rows(T, families)
    rows = len(families)
    P = torch.full((rows + 2, T), BF16_CANARY, dtype=torch.int16, device="cuda")
    sd = _dev(s)
    check(lib.natinf_debug_softmax_rows(kind, ptr(sd), ptr(P) + 2 * T, T, rows, stream_ptr()), "natinf_debug_softmax_rows")
    torch.cuda.synchronize()
    out = P.cpu().numpy().view(np.uint16)
    assert np.all(out[0] == BF16_CANARY) and np.all(out[-1] == BF16_CANARY), "a canary row around P was written"
    bad, ratio = R.check_softmax(s, families, out[1:-1])
    print(f"\nsoftmax kind {kind} T {T} rows {rows} {families if rows == 1 else ''}: worst (|P - p| - half ulp - floor) / (eps p) = {ratio:.3f}")
    assert not bad, f"rows {bad} ({[families[i] for i in bad]}) outside the radius"
