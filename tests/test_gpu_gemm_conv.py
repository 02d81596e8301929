"""The plain GEMM kernels in implicit 3x3-convolution mode (taps == 9: a zero-bordered [B][H+2][W+2][C] operand, an optional 1x1
shortcut segment a1) on their own, through natinf_debug_gemm / natinf_debug_gemm_fused, against an fp64 reference of nine shifted
matmuls.  This is every 3x3 convolution that does not go through the fused GroupNorm kernels: the AutoencoderKL decoder, the unfused
NCSN++ convolutions and the split-K path of the 8x8 / 4x4 levels.

Exact-integer mode (the main check): activations and weights are small integers, the bias is an integer and the scale a power of two.
Every product and every partial sum is then an integer (times the scale) far below 2^24, so any fp32 summation order gives the exact
result and the kernel must equal the fp64 reference cast to the output type, bit for bit: one dropped or doubled K term fails.
Random-normal mode checks realistic magnitudes against the elementwise fp32 accumulation bound.  Guard bands: the output starts as NaN
and has a tail that must come back untouched; the operands are cut out of NaN-filled buffers, so a read past an end shows up as NaN."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

V_AUTO, V_GENERIC, V_RING64, V_RING256W4, V_DMA128P, V_DMA256H, V_DMA512H = 0, 1, 8, 9, 17, 26, 27
TILE_VARIANT = {"generic128": V_GENERIC, "ring64x128": V_RING64, "ring256x128w4": V_RING256W4, "dma128x128p": V_DMA128P,
                "dma256x256h": V_DMA256H, "dma512x128h": V_DMA512H}
NATINF_EINVAL = -1
GUARD = 4096            # elements of NaN in front of / behind every operand and behind every output


# ---------------------------------------------------------------------------------------------------------------------------------
# layout helpers and the reference (device-agnostic: tests/test_gemm_conv_host.py checks them against F.conv2d on the CPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def pad_nhwc(x):
    """NCHW -> the zero-bordered [B][H+2][W+2][C] operand of a taps == 9 launch"""
    B, Cc, H, W = x.shape
    a = torch.zeros(B, H + 2, W + 2, Cc, dtype=x.dtype, device=x.device)
    a[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    return a


def pack_weights(w, w1=None):
    """[N][C][3][3] (+ [N][C1]) -> the engine's K order: ((c / 64) * 9 + tap) * 64 + c % 64, tap = 3 ky + kx, then the shortcut columns"""
    N, Cc = w.shape[:2]
    p = w.reshape(N, Cc // 64, 64, 9).permute(0, 1, 3, 2).reshape(N, 9 * Cc)
    return torch.cat([p, w1], dim=1).contiguous() if w1 is not None else p.contiguous()


def conv_ref(a_pad, wp, a1=None, bias=None, scale=1.0, dtype=torch.float64):
    """sum over the nine taps of shifted [M][C] views of the zero-bordered operand times that tap's [N][C] block of the PACKED weights
    (+ a1 @ w1^T + bias) * scale, in `dtype`; no im2col.  Returns [M][N] with m = (b * H + y) * W + x."""
    B, Hp, Wp, Cc = a_pad.shape
    H, W = Hp - 2, Wp - 2
    N = wp.shape[0]
    wt = wp[:, :9 * Cc].to(dtype).reshape(N, Cc // 64, 9, 64).permute(2, 0, 1, 3).reshape(9, N, Cc)      # [tap][N][C]
    out = torch.zeros(B * H * W, N, dtype=dtype, device=a_pad.device)
    for t in range(9):
        ky, kx = divmod(t, 3)
        out += a_pad[:, ky:ky + H, kx:kx + W, :].to(dtype).reshape(-1, Cc) @ wt[t].t()
    if a1 is not None:
        out += a1.to(dtype) @ wp[:, 9 * Cc:].to(dtype).t()
    if bias is not None:
        out += bias.to(dtype)
    return out * scale


# ---------------------------------------------------------------------------------------------------------------------------------
# operands with guard bands
# ---------------------------------------------------------------------------------------------------------------------------------
def _guarded(n, dtype, dev="cuda"):
    """a flat NaN buffer with GUARD elements on both sides; returns (buffer, view of the n middle elements)"""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _ints(shape, lo, hi, g, dev="cuda"):
    return torch.randint(lo, hi + 1, shape, generator=g, device=dev).float()


def _operands(B, res, cin, N, K1, mode, seed, lo=-3, hi=3):
    """bf16 operands in guarded buffers: a_pad [B][res+2][res+2][cin], a1 [M][K1] or None, wp [N][9 cin + K1], bias [N] fp32"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    M = B * res * res
    if mode == "int":
        x, w = _ints((B, cin, res, res), lo, hi, g), _ints((N, cin, 3, 3), lo, hi, g)
        s1, w1 = (_ints((M, K1), lo, hi, g), _ints((N, K1), lo, hi, g)) if K1 else (None, None)
        bias = _ints((N,), -8, 8, g)
    else:
        x, w = torch.randn(B, cin, res, res, generator=g, device="cuda"), torch.randn(N, cin, 3, 3, generator=g, device="cuda")
        s1, w1 = (torch.randn(M, K1, generator=g, device="cuda"), torch.randn(N, K1, generator=g, device="cuda")) if K1 else (None, None)
        bias = torch.randn(N, generator=g, device="cuda")
    a_pad = pad_nhwc(x.bfloat16())
    abuf, av = _guarded(a_pad.numel(), torch.bfloat16)
    av.copy_(a_pad.reshape(-1))
    a_pad = av.view(a_pad.shape)
    wp = pack_weights(w.bfloat16(), w1.bfloat16() if K1 else None)
    bbuf, bv = _guarded(wp.numel(), torch.bfloat16)
    bv.copy_(wp.reshape(-1))
    wp = bv.view(wp.shape)
    a1 = a1buf = None
    if K1:
        a1buf, v1 = _guarded(M * K1, torch.bfloat16)
        v1.copy_(s1.bfloat16().reshape(-1))
        a1 = v1.view(M, K1)
    return dict(a_pad=a_pad, a1=a1, wp=wp, bias=bias, keep=(abuf, bbuf, a1buf))


def _out(n, f32):
    buf, v = _guarded(n, torch.float32 if f32 else torch.bfloat16)
    return buf, v


def _tail_intact(buf, n):
    """the NaN guard behind an output of n elements came back bit for bit"""
    w = torch.int32 if buf.dtype == torch.float32 else torch.int16
    ref = torch.full((GUARD,), float("nan"), dtype=buf.dtype, device=buf.device).view(w)
    return torch.equal(buf[GUARD + n:].view(w), ref) and torch.equal(buf[:GUARD].view(w), ref)


def _profile(fn):
    """runs fn() with natinf_gemm_profile on; returns fn's result and the kernel tags of the launches it made (profile_read rows)"""
    from naturaldiffusion_amd._lib import lib, check
    buf = C.create_string_buffer(1 << 16)
    lib.natinf_gemm_profile_read(buf, len(buf))                     # drop anything recorded before
    try:
        check(lib.natinf_gemm_profile(1), "profile on")
        r = fn()
        torch.cuda.synchronize()
    finally:
        check(lib.natinf_gemm_profile(0), "profile off")
    n = lib.natinf_gemm_profile_read(buf, len(buf))
    assert n >= 0, n
    return r, [ln.split() for ln in buf.value.decode().splitlines()]


def _splitk_ws(slices, M, N):
    from naturaldiffusion_amd._lib import lib, check, ptr
    ws = torch.full((slices * M * N,), float("nan"), device="cuda") if slices else None
    check(lib.natinf_debug_set_splitk_workspace(ptr(ws) if slices else None, slices), "set_splitk_workspace")
    return ws


def run_conv(variant, B, res, N, op, c_f32, scale, splitk=0):
    """one natinf_debug_gemm launch in 3x3 mode; returns (output [M][N] fp32 view, output buffer, kernel tag)"""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    cin, M = op["a_pad"].shape[-1], B * res * res
    K1 = op["a1"].shape[1] if op["a1"] is not None else 0
    buf, c = _out(M * N, c_f32)
    ws = _splitk_ws(splitk, M, N)
    try:
        rc, rows = _profile(lambda: lib.natinf_debug_gemm(variant, M, N, 9 * cin, K1, 9, res.bit_length() - 1, 1, ptr(op["a_pad"]),
                                                          ptr(op["a1"]) if K1 else None, ptr(op["wp"]), ptr(op["bias"]), ptr(c),
                                                          int(c_f32), scale, 1, stream_ptr()))
    finally:
        _splitk_ws(0, 0, 0)
    check(rc, "debug_gemm")
    del ws
    assert len(rows) == 1 and rows[0][:6] == [str(M), str(N), str(9 * cin), str(K1), "9", "1"], rows
    return c.view(M, N), buf, rows[0][6].split("/")[0]


def _ref_of(op, scale, dtype=torch.float64):
    return conv_ref(op["a_pad"], op["wp"], op["a1"], op["bias"], scale, dtype)


def _expect_exact(got, ref64, c_f32):
    want = ref64.float() if c_f32 else ref64.to(torch.bfloat16)
    if torch.equal(got, want):
        return
    bad = (got.float() != want.float()).nonzero()
    m, n = bad[0].tolist()
    raise AssertionError(f"{len(bad)} outputs differ; first at m={m} n={n}: got {got[m, n].item()} want {want[m, n].item()} "
                         f"(fp64 {ref64[m, n].item()})")


# ---------------------------------------------------------------------------------------------------------------------------------
# exact-integer mode
# ---------------------------------------------------------------------------------------------------------------------------------
CASES = [   # (variant, B, res, cin, N, K1, fp32 output, the tile that must run)
    (V_RING64, 5, 4, 64, 136, 0, False, "ring64x128"),              # 4x4: a 64-row tile spans 4 images; 5 images = a ragged last tile
    (V_RING64, 7, 8, 128, 264, 64, True, "ring64x128"),             # shortcut K1 != cin
    (V_RING64, 2, 32, 256, 256, 256, False, "ring64x128"),
    (V_RING256W4, 5, 8, 256, 128, 256, False, "ring256x128w4"),     # 8x8: a 256-row tile spans 4 images
    (V_RING256W4, 7, 4, 64, 392, 0, True, "ring256x128w4"),         # 4x4: 16 images per tile, 7 in all
    (V_RING256W4, 2, 16, 512, 256, 512, False, "ring256x128w4"),    # widest K: 4608 + 512
    (V_DMA128P, 3, 16, 128, 256, 128, False, "dma128x128p"),
    (V_DMA128P, 5, 4, 512, 136, 0, True, "dma128x128p"),
    (V_DMA128P, 1, 64, 64, 264, 64, False, "dma128x128p"),
    (V_DMA256H, 2, 32, 64, 264, 0, False, "dma256x256h"),           # K = 576: not a multiple of the 128 / 256-wide K schedule
    (V_DMA256H, 7, 8, 256, 392, 128, True, "dma256x256h"),
    (V_DMA256H, 1, 256, 64, 256, 0, False, "dma256x256h"),          # 256x256 images
    (V_DMA512H, 1, 64, 64, 128, 64, False, "dma512x128h"),
    (V_DMA512H, 5, 8, 128, 136, 0, True, "dma512x128h"),            # a 512-row tile spans 8 images
    (V_DMA512H, 3, 16, 256, 128, 256, False, "dma512x128h"),
    (V_AUTO, 1, 512, 128, 128, 0, False, None),                     # the VAE's last level: 512x512
    (V_AUTO, 7, 4, 256, 256, 256, False, None),
    (V_AUTO, 3, 32, 128, 256, 128, True, None),
    (V_AUTO, 3, 8, 64, 136, 32, False, "generic128"),               # K1 % 64 != 0: the generic kernel on the padded operand
    (V_AUTO, 2, 16, 128, 256, 32, True, "generic128"),
]


@pytest.mark.parametrize("variant,B,res,cin,N,K1,c_f32,tile", CASES)
def test_conv_exact_integers(variant, B, res, cin, N, K1, c_f32, tile):
    op = _operands(B, res, cin, N, K1, "int", seed=B * 1000 + res + cin + N + K1)
    got, buf, ran = run_conv(variant, B, res, N, op, c_f32, 0.5)
    torch.cuda.synchronize()
    if tile is not None:
        assert ran == tile, (ran, tile)                         # a forced variant that fell back is not the case it claims to be
    _expect_exact(got, _ref_of(op, 0.5), c_f32)
    assert _tail_intact(buf, got.numel())


# ---------------------------------------------------------------------------------------------------------------------------------
# random-normal mode: one case per kernel, elementwise fp32 accumulation bound
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,B,res,cin,N,K1,c_f32", [
    (V_RING64, 3, 8, 128, 136, 64, False), (V_RING256W4, 2, 16, 256, 256, 0, True), (V_DMA128P, 5, 4, 128, 264, 128, False),
    (V_DMA256H, 1, 32, 128, 256, 128, True), (V_DMA512H, 2, 16, 64, 128, 0, False), (V_AUTO, 3, 8, 64, 136, 32, True),
])
def test_conv_random_normal_within_the_accumulation_bound(variant, B, res, cin, N, K1, c_f32):
    op = _operands(B, res, cin, N, K1, "randn", seed=7 + variant)
    scale = 0.25
    got, buf, ran = run_conv(variant, B, res, N, op, c_f32, scale)
    if variant != V_AUTO:
        assert TILE_VARIANT[ran] == variant, ran
    else:
        assert ran == "generic128", ran
    ref = _ref_of(op, scale)
    absop = dict(a_pad=op["a_pad"].abs(), wp=op["wp"].abs(), a1=op["a1"].abs() if K1 else None, bias=op["bias"].abs())
    mag = _ref_of(absop, scale)
    K = 9 * cin + K1
    tol = (K + 1) * 2.0 ** -24 * mag
    if not c_f32:
        tol = tol + 2.0 ** -8 * (ref.abs() + tol)                # + half an ulp of bf16
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all()
    assert (err <= tol).all(), (err - tol).max().item()
    assert _tail_intact(buf, got.numel())


# ---------------------------------------------------------------------------------------------------------------------------------
# split-K with taps == 9
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,res,cin,N,K1", [
    (32, 4, 256, 256, 0),         # K = 2304, 4 slices of 18 K-tiles
    (8, 8, 256, 256, 768),        # 96 K-tiles / 4: a slice boundary exactly at the end of the 3x3 segment (K = 2304)
    (8, 8, 256, 256, 1280),       # 112 K-tiles / 4: the last boundary inside the shortcut segment
    (32, 4, 512, 256, 0),         # K = 4608
])
def test_conv_splitk_exact_and_equal_to_the_unsplit_launch(B, res, cin, N, K1):
    op = _operands(B, res, cin, N, K1, "int", seed=res * 100 + K1)
    got, buf, ran = run_conv(V_AUTO, B, res, N, op, False, 0.5, splitk=4)
    assert ran == "splitk4_ring128x128", ran
    _expect_exact(got, _ref_of(op, 0.5), False)
    assert _tail_intact(buf, got.numel())
    again, _, _ = run_conv(V_AUTO, B, res, N, op, False, 0.5, splitk=4)
    assert torch.equal(again, got)                               # deterministic
    unsplit, _, ran1 = run_conv(V_AUTO, B, res, N, op, False, 0.5)
    assert not ran1.startswith("splitk")
    assert torch.equal(unsplit, got)


# ---------------------------------------------------------------------------------------------------------------------------------
# batch > 1, taps == 1 (the NCSN++ attention's batched products) against torch.bmm
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,batch,M,N,K", [(V_AUTO, 512, 256, 256, 256), (V_RING256W4, 512, 256, 256, 256),
                                                 (V_DMA128P, 7, 200, 136, 192), (V_RING64, 5, 130, 264, 64)])
def test_batched_plain_gemm_against_bmm(variant, batch, M, N, K):
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    g = torch.Generator(device="cuda").manual_seed(batch + M)
    a, b = _ints((batch, M, K), -3, 3, g).bfloat16(), _ints((batch, N, K), -3, 3, g).bfloat16()
    bias = _ints((N,), -8, 8, g)
    abuf, av = _guarded(a.numel(), torch.bfloat16); av.copy_(a.reshape(-1))
    bbuf, bv = _guarded(b.numel(), torch.bfloat16); bv.copy_(b.reshape(-1))
    buf, c = _out(batch * M * N, False)
    rc, rows = _profile(lambda: lib.natinf_debug_gemm(variant, M, N, K, 0, 1, 0, batch, ptr(av), None, ptr(bv), ptr(bias), ptr(c), 0,
                                                      0.5, 1, stream_ptr()))
    check(rc, "debug_gemm")
    if variant != V_AUTO:
        assert TILE_VARIANT[rows[0][6].split("/")[0]] == variant, rows
    else:
        assert rows[0][6].startswith("ring256x128w4/"), rows         # the profile's "16x16x256 batch 512" line
    ref = (torch.bmm(a.double(), b.double().transpose(1, 2)) + bias.double()) * 0.5
    _expect_exact(c.view(batch * M, N), ref.reshape(batch * M, N), False)
    assert _tail_intact(buf, c.numel())


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: each returns NATINF_EINVAL before anything is launched
# ---------------------------------------------------------------------------------------------------------------------------------
def test_debug_gemm_refuses_undefined_launches():
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    a = torch.zeros(1 << 20, dtype=torch.bfloat16, device="cuda")
    c = torch.full((1 << 20,), float("nan"), device="cuda")
    p = ptr(a)

    def gemm(variant=V_AUTO, M=64, N=136, K0=576, K1=0, taps=9, logW=3, batch=1, a1=None):
        return lib.natinf_debug_gemm(variant, M, N, K0, K1, taps, logW, batch, p, a1, p, None, ptr(c), 0, 1.0, 1, stream_ptr())

    assert gemm() == 0                                           # the well-formed launch the others differ from
    torch.cuda.synchronize()
    assert gemm(K0=9 * 32) == NATINF_EINVAL                      # 3x3 with 32 channels: no defined K order
    assert gemm(K0=9 * 96, variant=V_DMA128P) == NATINF_EINVAL
    assert gemm(K0=9 * 32, K1=64, a1=p) == NATINF_EINVAL
    assert gemm(K0=577) == NATINF_EINVAL                         # K0 % taps
    assert gemm(taps=1, K0=136, logW=0, M=64) == 0               # (taps == 1: K0 % 64 != 0 is fine, the generic kernel)
    assert gemm(N=132) == NATINF_EINVAL                          # ragged N on a row-major output
    assert gemm(N=3) == NATINF_EINVAL
    assert gemm(taps=1, K0=128, logW=0, N=12) == NATINF_EINVAL
    assert gemm(batch=2) == NATINF_EINVAL                        # 3x3 with batch > 1
    assert gemm(M=96) == NATINF_EINVAL                           # not whole 8x8 images
    assert gemm(K1=64) == NATINF_EINVAL                          # K1 without a1
    torch.cuda.synchronize()
    assert torch.isnan(c[64 * 136:]).all()                       # nothing but the first launch wrote


def test_fused_conv_hook_refusals_and_one_shot():
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    a = torch.zeros(1 << 20, dtype=torch.bfloat16, device="cuda")
    c = torch.full((1 << 20,), float("nan"), device="cuda")
    p, bm = ptr(a), C.c_int(0)

    def fused(M=64, N=8, K=576, c_f32=1, rowvec=None, logW=3, a1=None, c1=0):
        if logW is not None:
            assert lib.natinf_debug_set_conv_operand(logW, a1, c1) == 0
        return lib.natinf_debug_gemm_fused(0, M, N, K, p, p, None, None, rowvec, None, 6, None, None, 1.0, 0, ptr(c), c_f32, None,
                                           C.byref(bm), 0, stream_ptr())

    assert lib.natinf_debug_set_conv_operand(-1, None, 0) == NATINF_EINVAL
    assert lib.natinf_debug_set_conv_operand(3, p, 32) == NATINF_EINVAL       # shortcut width % 64
    assert lib.natinf_debug_set_conv_operand(3, None, 64) == NATINF_EINVAL
    assert fused(K=9 * 32) == NATINF_EINVAL
    assert fused(K=577) == NATINF_EINVAL
    assert fused(M=96) == NATINF_EINVAL
    assert fused(N=3) == NATINF_EINVAL                           # ragged N, row-major
    assert fused(N=3, c_f32=2, rowvec=p) == NATINF_EINVAL        # NCHW carries bias and scale only
    assert fused(N=3, c_f32=2, logW=None) == NATINF_EINVAL       # NCHW needs the conv operand: the hook was consumed by the last call
    assert fused(N=3, c_f32=3) == NATINF_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(c).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused epilogue terms in 3x3 mode (natinf_debug_set_conv_operand + natinf_debug_gemm_fused)
# ---------------------------------------------------------------------------------------------------------------------------------
def run_fused_conv(variant, B, res, N, op, rowvec=None, resid=None, gn=False, c_f32=0, scale=1.0, splitk=0):
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    cin, M = op["a_pad"].shape[-1], B * res * res
    K1 = op["a1"].shape[1] if op["a1"] is not None else 0
    buf, c = _out(M * N, c_f32)
    part = torch.full((((M + 15) // 16) * (N // 4) * 2,), float("nan"), device="cuda") if gn else None
    ws = _splitk_ws(splitk, M, N)
    bm = C.c_int(0)
    lrs = 2 * (res.bit_length() - 1)

    def go():
        check(lib.natinf_debug_set_conv_operand(res.bit_length() - 1, ptr(op["a1"]) if K1 else None, K1), "set_conv_operand")
        return lib.natinf_debug_gemm_fused(variant, M, N, 9 * cin, ptr(op["a_pad"]), ptr(op["wp"]), ptr(op["bias"]), None,
                                           ptr(rowvec) if rowvec is not None else None, None, lrs, ptr(resid) if resid is not None else None,
                                           None, scale, 0, ptr(c), c_f32, ptr(part) if gn else None, C.byref(bm), 0, stream_ptr())
    try:
        rc, rows = _profile(go)
    finally:
        _splitk_ws(0, 0, 0)
    check(rc, "debug_gemm_fused")
    del ws
    assert len(rows) == 1, rows
    return c, buf, part, bm.value, rows[0][6]


@pytest.mark.parametrize("B,res,cin,N,K1,use_resid,gn,splitk", [
    (512, 16, 256, 256, 0, True, True, 0),        # 16x16 unfused shape: per-sample row vector, residual, GroupNorm partials
    (512, 16, 256, 256, 256, False, True, 0),     # ... with the shortcut segment
    (512, 8, 256, 256, 0, True, False, 4),        # 8x8 at B = 512 (no split: enough tiles)
    (128, 8, 256, 256, 256, False, True, 4),      # 8x8 split-K: the reduce pass writes 16-row partials
    (512, 4, 256, 256, 0, True, True, 4),         # 4x4 split-K
    (512, 4, 512, 256, 0, False, False, 4),
])
def test_fused_terms_in_conv_mode_exact(B, res, cin, N, K1, use_resid, gn, splitk):
    M, HW = B * res * res, res * res
    # values in [-1, 1]: the outputs stay small enough for the GroupNorm sums of squares to be exact in fp32 too (checked below)
    op = _operands(B, res, cin, N, K1, "int", seed=res + N + K1 + B, lo=-1, hi=1)
    g = torch.Generator(device="cuda").manual_seed(5)
    rowvec = _ints((B, N), -16, 16, g)
    resid = _ints((M, N), -4, 4, g).bfloat16() if use_resid else None
    scale = 0.5
    c, buf, part, bm, tag = run_fused_conv(V_AUTO, B, res, N, op, rowvec, resid, gn, 0, scale, splitk)
    v = conv_ref(op["a_pad"], op["wp"], op["a1"], op["bias"], 1.0)
    v += rowvec.double().repeat_interleave(HW, dim=0)
    if use_resid:
        v += resid.double()
    v *= scale
    _expect_exact(c.view(M, N), v, False)
    assert _tail_intact(buf, M * N)
    if gn:
        assert HW % bm == 0, (bm, HW, tag)                       # a partial tile inside one sample
        t = v.reshape(M // bm, bm, N // 4, 4)
        s, q = t.sum(dim=(1, 3)), (t * t).sum(dim=(1, 3))
        assert q.max().item() < 2 ** 22 and t.abs().sum(dim=(1, 3)).max().item() < 2 ** 22    # exact in fp32 in any order (multiples of 1/4)
        got = part[:(M // bm) * (N // 4) * 2].view(M // bm, N // 4, 2).double()
        assert torch.equal(got[..., 0], s) and torch.equal(got[..., 1], q), tag


@pytest.mark.parametrize("B,res,variant", [(2, 64, V_AUTO), (3, 64, V_DMA128P), (1, 512, V_AUTO)])
def test_vae_head_nchw_exact(B, res, variant):
    """the decoder's 128 -> 3 output head: an N = 3 launch writing fp32 NCHW"""
    M, HW, N = B * res * res, res * res, 3
    op = _operands(B, res, 128, N, 0, "int", seed=res + B)
    c, buf, _, _, tag = run_fused_conv(variant, B, res, N, op, c_f32=2, scale=0.5)
    if variant != V_AUTO:
        assert TILE_VARIANT[tag.split("/")[0]] == variant, tag
    want = _ref_of(op, 0.5).float().reshape(B, HW, N).permute(0, 2, 1).reshape(-1)
    assert torch.equal(c, want)
    assert _tail_intact(buf, M * N)


# ---------------------------------------------------------------------------------------------------------------------------------
# the engines' own 3x3 shapes, collected at run time
# ---------------------------------------------------------------------------------------------------------------------------------
def _engine_conv_lines():
    """every taps == 9 launch of the NCSN++ plan at B = 512 (default and natinf_set_fuse_gn(0)) that is not a fused GroupNorm
    convolution or the fused head, and every 3x3 launch of a small AutoencoderKL decode (natinf_gemm_profile): (M, N, K0, K1, tile)"""
    from naturaldiffusion_amd._lib import lib, check
    from naturaldiffusion_amd.ncsnpp import NCSNppEngine, flatten_state_dict
    from naturaldiffusion_amd.synth import synthetic_state_dict
    from naturaldiffusion_amd.vae import VAEDecoder, flatten_state_dict as flat_vae
    from oracle import vae_oracle as V
    flat = flatten_state_dict(synthetic_state_dict(0))
    lines = []
    for fuse in (1, 0):
        try:
            check(lib.natinf_set_fuse_gn(fuse), "set_fuse_gn")
            eng = NCSNppEngine(flat, max_batch=2, device="cuda:0")
        finally:
            check(lib.natinf_set_fuse_gn(1), "set_fuse_gn")
        lines += [("ncsnpp", r) for r in eng.describe_gemms(512)]
        del eng
    dec = VAEDecoder(flat_vae(V.make_params(4, seed=3), 4), max_batch=1, latent_ch=4, latent_res=8)
    z = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(0)).cuda()
    _, rows = _profile(lambda: dec(z))
    lines += [("vae", r) for r in rows]
    out = {}
    for src, r in lines:
        M, N, K0, K1, taps, batch = (int(x) for x in r[:6])
        tile = r[6].split("/")[0]
        if taps != 9 or tile.startswith("conv_gn") or tile.startswith("head_conv"):
            continue
        out.setdefault((src, M, N, K0, K1), set()).add(tile)
    return out


def test_engine_conv_shapes_exact():
    """each engine shape through the debug entry at the engine's M: once with the automatic choice (split-K workspace given, as the
    engines give one), once forced onto every tile the engine itself ran it on; the union of tiles run covers every engine 3x3 tile"""
    shapes = _engine_conv_lines()
    assert any(s[0] == "ncsnpp" for s in shapes) and any(s[0] == "vae" for s in shapes), shapes
    engine_tiles, ran_tiles = set(), set()
    for (src, M, N, K0, K1), tiles in sorted(shapes.items()):
        cin = K0 // 9
        engine_tiles |= tiles
        res = None
        for r in (4, 8, 16, 32, 64, 128, 256, 512):
            if src == "vae" and r * r == M or src == "ncsnpp" and 512 * r * r == M:
                res = r
        assert res is not None, (src, M)
        B = M // (res * res)
        op = _operands(B, res, cin, N, K1, "int", seed=M + N + K0 + K1)
        ref = _ref_of(op, 0.5)
        if N % 8:                                                  # the VAE head (N = 3): the NCHW output
            for tile in tiles | {"auto"}:
                c, buf, _, _, tag = run_fused_conv(TILE_VARIANT.get(tile, V_AUTO), B, res, N, op, c_f32=2, scale=0.5)
                ran_tiles.add(tag.split("/")[0])
                assert torch.equal(c, ref.float().reshape(B, res * res, N).permute(0, 2, 1).reshape(-1)), (src, M, N, K0, K1, tag)
                assert _tail_intact(buf, M * N)
            continue
        for tile in sorted(tiles | {"auto"}):
            variant = V_AUTO if tile == "auto" or tile.startswith("splitk") else TILE_VARIANT[tile]
            splitk = 4 if variant == V_AUTO and res <= 8 else 0
            got, buf, ran = run_conv(variant, B, res, N, op, False, 0.5, splitk=splitk)
            if tile != "auto":
                assert ran == tile, (src, M, N, K0, K1, ran, tile)
            ran_tiles.add(ran)
            _expect_exact(got, ref, False)
            assert _tail_intact(buf, M * N)
        del op, ref
    assert engine_tiles <= ran_tiles, (engine_tiles, ran_tiles)
    print("\nengine 3x3 shapes (source, M, N, K0, K1): tiles --", "; ".join(f"{k}: {sorted(v)}" for k, v in sorted(shapes.items())))
    print("engine 3x3 tiles:", sorted(engine_tiles), "| tiles run:", sorted(ran_tiles))
