"""The GroupNorm partial sums of the packed tile epilogue (csrc/gemm_dma.h, packed_tile_epilogue: since round 8 a lane keeps them as packed fp32 pairs -- even / odd columns
of its four -- and folds x + y once in front of the DPP row sums) on every instantiation that carries them: k_conv_gn2 at 32x32 / 16x16 / 8x8 / 4x4 (one, two and four
samples per tile, ragged last tiles), the three k_conv_gn3 tiles, the up-fold launch and the plain k_gemm_dma tiles; and the consumer's GroupNorm table where the tile writes
it itself (natinf_debug_conv_gn_fin: 16x16 on k_conv_gn3, 8x8 / 4x4 on k_conv_gn2).

Two kinds of data per case:
  * random: the (sum, sum of squares) table against float64 of the same op, 5e-3 of max |want| (the bound tests/test_gpu_conv_gn.py / test_gpu_conv_gn3.py / test_gpu_up_fold.py
    hold these tables to); the producer-written table against the float64 GroupNorm of the reference output, 5e-3 of max |table|;
  * exact: integers times 0.5 -- every output is a multiple of 1/2, every square a multiple of 1/4, every sum below 2^22 (asserted), so ANY fp32 summation order gives the
    exact sums: the table must equal float64 BIT FOR BIT.  (The fused convolutions round their activated operand, so their 3x3 weights are zero there and the integers
    come in through the 1x1 shortcut segment, the bias and the residual; the up-fold launch takes x in {0, 32}, where SiLU is the identity in fp32.)  With exact sums the
    producer-written table is eight correctly rounded fp32 operations away from float64: 1e-5 of max |table|.
The output tensor must not move at all: on exact data it equals float64 rounded to bf16; on random data it equals, byte for byte, the same launch WITHOUT the statistics
(epilogues 1 / 5: instantiations the packed sums are not part of)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634
GN_EPS = 1e-6
_DEFAULT_MASK, _DEFAULT_MIN_K = 7, (2304, 0, 2304)          # (csrc/gemm_launch.h: g_cg3, g_cg3_min_k)


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _pack(w, w1):
    N, Cc = w.shape[:2]
    p = w.reshape(N, Cc // 64, 64, 9).permute(0, 1, 3, 2).reshape(N, 9 * Cc)
    return torch.cat([p, w1], dim=1).contiguous() if w1 is not None else p.contiguous()


def _conv_case(res, B, cin, N, resid, exact, seed):
    """operands of natinf_debug_conv_gn and the float64 result [B res res][N]"""
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.bfloat16().float()
    M = B * res * res
    x = bf(torch.randn(B, res, res, cin, generator=g))
    scale = torch.rand(B, cin, generator=g) * 1.5 + 0.25
    shift = torch.randn(B, cin, generator=g) * 0.5
    if exact:
        c1, out_scale = 128, 0.5                   # (the 4x4 tile splits K over two groups: shortcut channels in multiples of 128)
        w = torch.zeros(N, cin, 3, 3)
        w1, a1 = _ints((N, c1), -1, 1, g), _ints((M, c1), -2, 2, g)
        bias = _ints((N,), -4, 4, g)
        r = _ints((M, N), -4, 4, g) if resid else None
        ref = a1.double() @ w1.double().t()
    else:
        c1, out_scale = 0, 0.70710678
        w = bf(torch.randn(N, cin, 3, 3, generator=g) / np.sqrt(9 * cin))
        w1 = a1 = None
        bias = torch.randn(N, generator=g) * 0.1
        r = bf(torch.randn(M, N, generator=g)) if resid else None
        h = bf(F.silu(x * scale[:, None, None, :] + shift[:, None, None, :]))
        ref = F.conv2d(h.permute(0, 3, 1, 2).double(), w.double(), padding=1).permute(0, 2, 3, 1).reshape(M, N)
    ref = ref + bias.double()
    if resid:
        ref = ref + r.double()
    return dict(x=x, scale=scale, shift=shift, w=w, w1=w1, a1=a1, bias=bias, r=r, c1=c1, out_scale=out_scale), ref * out_scale


def _run_conv(res, B, cin, N, t, mask, rows, parts, fin):
    """-> out [M][N] bf16, part [B-or-tiles + 2][N / 4][2] (two sentinel rows behind the last one), (fin_scale, fin_shift) [B + 1][N] (one sentinel row)"""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    dev, M, c1 = "cuda", B * res * res, t["c1"]
    wd = _pack(t["w"] * (-1.0 / LOG2E), t["w1"]).bfloat16().to(dev)
    xd = t["x"].bfloat16().to(dev).contiguous()
    scd, shd, bd = (t["scale"] * -LOG2E).to(dev), (t["shift"] * -LOG2E).to(dev), t["bias"].to(dev)
    a1d = t["a1"].bfloat16().to(dev).contiguous() if c1 else None
    rd = t["r"].bfloat16().to(dev) if t["r"] is not None else None
    wf = torch.zeros_like(wd)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    part = torch.full((M // rows + 2, N // 4, 2), -1.0, device=dev) if parts else None
    tabs = None
    if fin is not None:
        gamma, beta, mul = fin
        gd, bed = gamma.to(dev), beta.to(dev)
        tabs = (torch.full((B + 1, N), -7.0, device=dev), torch.full((B + 1, N), -7.0, device=dev))
        check(lib.natinf_debug_conv_gn_fin(ptr(tabs[0]), ptr(tabs[1]), ptr(gd), ptr(bed), N // 32, mul), "fin")
    check(lib.natinf_set_conv_gn_w128(mask), "knob")
    for sh in range(3):
        check(lib.natinf_set_conv_gn_w128_min_k(sh, 0), "min_k")               # every K: the mask alone chooses between k_conv_gn3 and k_conv_gn2
    try:
        check(lib.natinf_debug_conv_gn(res, B, N, cin, c1, ptr(xd), ptr(scd), ptr(shd), ptr(wd), ptr(wf), ptr(a1d), ptr(bd), ptr(rd), t["out_scale"], ptr(out),
                                       ptr(part), 1, stream_ptr()), "conv_gn")
        torch.cuda.synchronize()
    finally:
        lib.natinf_debug_conv_gn_fin(None, None, None, None, 0, 1.0)
        lib.natinf_set_conv_gn_w128(_DEFAULT_MASK)
        for sh, k in enumerate(_DEFAULT_MIN_K):
            lib.natinf_set_conv_gn_w128_min_k(sh, k)
    return out.cpu(), (part.cpu() if parts else None), (tuple(x_.cpu() for x_ in tabs) if tabs else None)


def _sums(ref, rows):
    """float64 (sum, sum of squares) per `rows` consecutive rows and 4-column quad"""
    M, N = ref.shape
    v = ref.reshape(M // rows, rows, N // 4, 4)
    return torch.stack([v.sum(dim=(1, 3)), (v * v).sum(dim=(1, 3))], dim=-1)


def _check_parts(part, want, exact, what):
    n = want.shape[0]
    assert torch.all(part[n:] == -1.0), f"{what}: a partial row behind the last tile / sample was written"
    got = part[:n].double()
    if exact:
        assert want.abs().max().item() < 2 ** 22, what                                   # multiples of 1/4 below 2^22: exact in fp32 in any order
        bad = int((got != want).sum())
        print(f"  {what}: exact sums, {bad} of {want.numel()} entries differ")
        assert bad == 0, (what, bad, (got - want).abs().max().item())
    else:
        err = ((got - want).abs().max() / want.abs().max()).item()
        print(f"  {what}: partial sums max-rel {err:.3e}")
        assert err <= 5e-3, (what, err)


def _check_tables(tabs, ref, B, HW, gamma, beta, mul, exact, what):
    N = ref.shape[1]
    v = ref.reshape(B, HW, N // 8, 8)                                                    # 32 groups of 8 channels at N = 256
    mean, msq = v.mean(dim=(1, 3)), (v * v).mean(dim=(1, 3))
    var = (msq - mean * mean).clamp_min(0)
    sc = (1.0 / torch.sqrt(var + GN_EPS)).repeat_interleave(8, dim=1) * gamma.double()
    want = (sc * mul, (beta.double() - mean.repeat_interleave(8, dim=1) * sc) * mul)
    for got, w_, name in zip(tabs, want, ("scale", "shift")):
        assert torch.all(got[B:] == -7.0), f"{what}: a table row behind the last sample was written"
        err = ((got[:B].double() - w_).abs().max() / w_.abs().max()).item()
        print(f"  {what}: producer-written {name} table max-rel {err:.3e}")
        assert err <= (1e-5 if exact else 5e-3), (what, name, err)


def _check_out(out, ref, exact, same_launch_without_statistics, what):
    assert torch.isfinite(out.float()).all(), what
    if exact:
        assert torch.equal(out.double(), ref.bfloat16().double()) and torch.equal(ref.bfloat16().double(), ref), what      # (representable: nothing to round)
    else:
        plain = same_launch_without_statistics()
        assert torch.equal(out.view(torch.int16), plain.view(torch.int16)), f"{what}: the statistics moved the output tensor"
        err = ((out.float() - ref.float()).abs().max() / ref.abs().max()).item()
        assert err <= 1e-2, (what, err)


CONV_CASES = [   # (res, B, cin, N, residual, k_conv_gn3 mask, rows per partial-sum row, producer-written table)
    (32, 1, 128, 128, False, 0, 256, False),      # k_conv_gn2, 256 x 128 tile, K = 1,152, epilogue 2
    (32, 3, 128, 128, True, 0, 256, False),       # ... epilogue 6, an odd batch
    (32, 1, 256, 128, False, 7, 512, False),      # k_conv_gn3<32, 4, 1>, K = 2,304
    (32, 1, 256, 256, False, 7, 256, False),      # k_conv_gn3<32, 2, 2>
    (16, 3, 256, 256, False, 7, 256, True),       # k_conv_gn3<16, 2, 2>, epilogue 2, with the table
    (16, 3, 256, 256, True, 7, 256, True),        # ... epilogue 6
    (16, 3, 256, 256, False, 0, 128, False),      # k_conv_gn2 at 16x16: the 128 x 256 tile
    (8, 3, 256, 256, False, 0, 64, True),         # two samples per tile, the last tile holds one
    (8, 3, 256, 256, True, 0, 64, True),
    (4, 5, 256, 256, False, 0, 16, True),         # four samples per tile, the last tile holds one
    (4, 5, 256, 256, True, 0, 16, True),
]


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("res,B,cin,N,resid,mask,rows,fin", CONV_CASES)
def test_fused_convolution_partial_sums_and_tables(res, B, cin, N, resid, mask, rows, fin, exact):
    what = f"res {res} B {B} N {N} resid {resid} mask {mask}"
    t, ref = _conv_case(res, B, cin, N, resid, exact, res * 100 + B * 10 + cin + N + resid + 7 * exact)
    g = torch.Generator().manual_seed(res + B)
    table = (torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.3, -LOG2E) if fin else None
    out, part, tabs = _run_conv(res, B, cin, N, t, mask, rows, True, table)
    _check_out(out, ref, exact, lambda: _run_conv(res, B, cin, N, t, mask, rows, False, None)[0], what)
    _check_parts(part, _sums(ref, rows), exact, what)
    if fin:
        _check_tables(tabs, ref, B, res * res, table[0], table[1], table[2], exact, what)


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
def test_up_fold_partial_sums(exact):
    """the up-fold launch (k_conv_gn_upfold: one 16x16 image x one output parity per tile), B = 2: row 4 s + 2 a + b of the table = sample s's pixels (2 i + a, 2 j + b)"""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    B, cin, N, dev = 2, 64, 256, "cuda"
    g = torch.Generator().manual_seed(41 + exact)
    bf = lambda t: t.bfloat16().float()
    if exact:
        # SiLU(0) = 0 and SiLU(32) = 32 / (1 + e^-32) = 32 in fp32; folded taps are sums of at most four +-1/32: every product is an integer
        x = 32.0 * (torch.rand(B, 16, 16, cin, generator=g) < 0.25).float()
        scale, shift = torch.ones(B, cin), torch.zeros(B, cin)
        w = _ints((N, cin, 3, 3), -1, 1, g) * (torch.rand(N, cin, 3, 3, generator=g) < 0.5).float() / 32.0
        bias, rowvec, out_scale = _ints((N,), -4, 4, g), _ints((B, N), -4, 4, g), 0.5
        h = x
    else:
        x = bf(torch.randn(B, 16, 16, cin, generator=g))
        scale, shift = torch.rand(B, cin, generator=g) * 1.5 + 0.25, torch.randn(B, cin, generator=g) * 0.5
        w = bf(torch.randn(N, cin, 3, 3, generator=g) / np.sqrt(9 * cin))
        bias, rowvec, out_scale = torch.randn(N, generator=g) * 0.1, torch.randn(B, N, generator=g) * 0.2, 0.70710678
        h = bf(F.silu(x * scale[:, None, None, :] + shift[:, None, None, :]))
    up = F.interpolate(h.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    ref = (F.conv2d(up.double(), w.double(), padding=1).permute(0, 2, 3, 1) + bias.double() + rowvec.double()[:, None, None, :]) * out_scale      # [B][32][32][N]

    def run(parts):
        xd, scd, shd, wd, bd, rvd = x.bfloat16().to(dev).contiguous(), scale.to(dev), shift.to(dev), w.to(dev).contiguous(), bias.to(dev), rowvec.to(dev).contiguous()
        wpk = torch.zeros(4 * N, 4 * cin, dtype=torch.bfloat16, device=dev)
        hs = torch.full((B, 18, 18, cin), float("nan"), dtype=torch.bfloat16, device=dev)
        out = torch.full((B * 1024, N), float("nan"), dtype=torch.bfloat16, device=dev)
        part = torch.full((4 * B + 2, N // 4, 2), -1.0, device=dev) if parts else None
        check(lib.natinf_debug_conv_up_fold(B, N, cin, ptr(xd), ptr(scd), ptr(shd), ptr(wd), ptr(wpk), ptr(hs), ptr(bd), ptr(rvd), out_scale, ptr(out), ptr(part), 1,
                                            stream_ptr()), "conv_up_fold")
        torch.cuda.synchronize()
        return out.cpu(), (part.cpu() if parts else None)

    out, part = run(True)
    _check_out(out, ref.reshape(B * 1024, N), exact, lambda: run(False)[0], "up-fold")
    want = torch.empty(B, 2, 2, N // 4, 2, dtype=torch.float64)
    for a in (0, 1):
        for b in (0, 1):
            ph = ref[:, a::2, b::2, :].reshape(B, 256, N // 4, 4)
            want[:, a, b, :, 0] = ph.sum(dim=(1, 3))
            want[:, a, b, :, 1] = (ph * ph).sum(dim=(1, 3))
    _check_parts(part, want.reshape(4 * B, N // 4, 2), exact, "up-fold")


V_DMA256P, V_DMA128P, V_DMA512 = 26, 17, 27        # (csrc/gemm_launch.h: the shipped k_gemm_dma tiles)
GEMM_CASES = [   # (variant, M, N, K, log2 rows per sample, fused terms)
    (V_DMA256P, 512, 264, 128, 8, ("bias_n", "rowvec", "gn")),               # epilogue 2, a ragged last column tile
    (V_DMA512, 1024, 128, 192, 9, ("bias_n", "rowvec", "resid", "gn")),      # epilogue 6 on the 512 x 128 tile
    (V_DMA128P, 384, 256, 64, 7, ("bias_n", "resid", "gn")),                 # epilogue 6 on the 128 x 128 tile
    (V_DMA128P, 300, 256, 64, 30, ("bias_n", "resid")),                      # epilogue 5, a partial last row tile (no statistics: the output alone)
]


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("variant,M,N,K,lrs,terms", GEMM_CASES)
def test_plain_gemm_partial_sums(variant, M, N, K, lrs, terms, exact):
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    dev = "cuda"
    g = torch.Generator().manual_seed(M + N + K + exact)
    ns = (M + (1 << lrs) - 1) >> lrs
    if exact:
        a, b = _ints((M, K), -2, 2, g), _ints((N, K), -1, 1, g)
        bias, rowvec, resid, scale = _ints((N,), -4, 4, g), _ints((ns, N), -4, 4, g), _ints((M, N), -4, 4, g), 0.5
    else:
        a, b = torch.randn(M, K, generator=g).bfloat16().float(), (torch.randn(N, K, generator=g) * 0.1).bfloat16().float()
        bias, rowvec, resid, scale = torch.randn(N, generator=g), torch.randn(ns, N, generator=g), torch.randn(M, N, generator=g).bfloat16().float(), 0.70710678
    has = lambda k: k in terms
    ref = a.double() @ b.double().t() + bias.double()
    if has("rowvec"):
        ref = ref + rowvec.double()[torch.arange(M) >> lrs]
    if has("resid"):
        ref = ref + resid.double()
    ref = ref * scale
    ad, bd, biasd, rvd, rsd = a.bfloat16().to(dev), b.bfloat16().to(dev), bias.to(dev), rowvec.to(dev), resid.bfloat16().to(dev)

    def run(gn, fp32_slab):
        c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
        part = torch.full((((M + 15) // 16) * (N // 4) * 2,), -1.0, device=dev) if gn else None
        bm = C.c_int(0)
        check(lib.natinf_debug_gemm_fused(variant, M, N, K, ptr(ad), ptr(bd), ptr(biasd), None, ptr(rvd) if has("rowvec") else None, None, lrs,
                                          ptr(rsd) if has("resid") else None, None, scale, 0, ptr(c), 0, ptr(part) if gn else None, C.byref(bm), int(fp32_slab),
                                          stream_ptr()), "debug_gemm_fused")
        torch.cuda.synchronize()
        return c.cpu(), (part.cpu() if gn else None), bm.value

    what = f"k_gemm_dma variant {variant} ({M}, {N}, {K}) {terms}"
    out, part, bm = run(has("gn"), False)
    # (without the statistics the launch takes epilogue 1 / 5; the statistics-free case is held to the general fp32-slab epilogue on exact data instead)
    _check_out(out, ref, exact, lambda: run(False, False)[0], what)
    if exact:
        assert torch.equal(out.view(torch.int16), run(has("gn"), True)[0].view(torch.int16)), f"{what}: packed and general epilogue differ"
    if has("gn"):
        assert M % bm == 0, (bm, what)
        _check_parts(part.reshape(-1, N // 4, 2)[: M // bm + 2], _sums(ref, bm), exact, what)
