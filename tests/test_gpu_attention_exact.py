"""The transformer attention kernels against answers that are known EXACTLY (tests/attention_exact_cases.py: `uniform` -- every key counted exactly once -- and
`selector` -- every query row picks one row of V), compared as bytes: k_flash_attn64 / k_flash_attn64_v2<1, 64> (natinf_attention_hd64_bf16, flash modes 0 and 3),
k_dit_flash<2,4 | 3,5 | 3,6> and k_attn_fused<., ., false, true> (natinf_dit_attention_bf16, streaming and NATINF_DIT_ATTN_RESIDENT) at every dispatch boundary of
the head width, in the wrappers' contiguous layouts and in the engines' interleaved ones with NaN canaries around the output; the fp8 output epilogue of the two
MMDiT kernels alone (natinf_debug_attention_hd64_fp8out); and the DiT engine at two head widths no other test builds.

Why equality holds on every kernel.  uniform: all scores are 0, every probability is exp2(0) = 1 (2^-8 after the resident kernel's normalisation at T = 256), the
row sum is the integer T, the numerator 1 or 0, and the byte of 1 / T does not depend on the form of the division (test_attention_exact_host.py).  selector: the
selected key's probability is exactly 1 where it is computed as exp2(s - s) (k_flash_attn64_v2, k_attn_fused) and 1 +- 2^-17 where the maximum is folded into an
fma against its own rounded product (k_flash_attn64, k_dit_flash: fma(s, c1, -(s c1))), in which case the bf16 numerator weight is 1.0 and the fp32 row sum carries
the 2^-17 -- 2^-8 of half a bf16 ulp; every other probability is below 2^-57.  No case here needed the one-ulp fallback."""
import functools

import numpy as np
import pytest
import torch

import attention_exact_cases as X
from test_gpu_dit512 import ATTN_TOL

pytestmark = pytest.mark.gpu

TOL = 3e-2          # max |engine - oracle| / max |oracle| (tests/test_gpu_dit.py, tests/test_gpu_dit512.py)
RESIDENT = 1        # NATINF_DIT_ATTN_RESIDENT


@pytest.fixture(params=[0, 1, 2, 3], ids=["online", "deferred", "deferred+mfma_sums", "deferred+mfma_sums_64key"])
def flash_mode(request):
    """every head_dim-64 attention kernel of the library (natinf_set_flash_mode), as in tests/test_gpu_mmdit.py"""
    from naturaldiffusion_amd._lib import lib, check
    rc = lib.natinf_set_flash_mode(request.param)
    if rc == -4 and request.param in (1, 2):                # NATINF_ESTATE
        pytest.skip("modes 1 / 2 (intermediate forms) are retired")
    check(rc, "natinf_set_flash_mode")
    yield request.param
    check(lib.natinf_set_flash_mode(3), "natinf_set_flash_mode")              # the library's default


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16 if a.dtype == np.uint16 else a.dtype)).cuda()


def _host16(t):
    return t.cpu().numpy().view(np.uint16)


# ---- natinf_attention_hd64_bf16 ----------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _mmdit_case(family, T):
    if family == "uniform":
        return X.uniform_case(2, max(2, -(-T // 128)), T, 64, seed=T)      # B H 64 >= T: every key owns a column (4,429: H = 35)
    return X.selector_case(2, 4 if T == 285 else 2, T, 64, seed=T)


def _run_mmdit(p):
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    q, vT, o = _dev(p["q"]), _dev(p["vT"]), _dev(p["o"])
    k = _dev(p["k"]) if "k" in p else None
    kptr = ptr(k) if k is not None else ptr(q) + 2 * p["k_off"]
    check(lib.natinf_attention_hd64_bf16(ptr(q), kptr, p["ld_qk"], p["qk_bs"], ptr(vT), ptr(o), p["ld_o"], p["o_bs"], p["B"], p["H"], p["Tp"], p["T"], 0.125,
                                         stream_ptr()), "natinf_attention_hd64_bf16")
    torch.cuda.synchronize()
    return _host16(o)


@pytest.mark.parametrize("engine_layout", [False, True], ids=["contiguous", "engine_layout"])
@pytest.mark.parametrize("T", [64, 65, 129, 285, 1100, 4429])
def test_mmdit_attention_counts_every_key_exactly_once(T, engine_layout, flash_mode):
    """uniform family.  Padded key rows hold 25.0 (as mmdit.attention_hd64 pads them) and the padded V^T columns 2^15: an admitted padded key is a gross error.
    engine_layout: one [B][Tp][2D] buffer with k = q + D (what the engine and bench.py pass), o with ld_o = D + 8 and a sequence stride of Tp + 3 rows -- the gap
    columns and rows must come back as the NaN canary they were filled with."""
    c = _mmdit_case("uniform", T)
    X.check_output(c, _run_mmdit(X.pack_mmdit(c, engine_layout=engine_layout)))


@pytest.mark.parametrize("engine_layout", [False, True], ids=["contiguous", "engine_layout"])
@pytest.mark.parametrize("T", [65, 129, 285, 4429])
def test_mmdit_attention_selects_the_permuted_value_row(T, engine_layout, flash_mode):
    """selector family: output row i of head h equals V[pi_h(i)] as bytes"""
    c = _mmdit_case("selector", T)
    X.check_output(c, _run_mmdit(X.pack_mmdit(c, engine_layout=engine_layout)))


@pytest.mark.parametrize("T", [65, 129, 285, 4429])
def test_mmdit_attention_ignores_nan_in_the_padded_key_rows(T, flash_mode):
    """include/natinf_mmdit.h: `keys >= T are ignored` -- whatever they hold.  Both kernels replace the masked scores by -inf with a select (flash_attn.h: `ok ?
    acc : -INFINITY`) before the maxima are taken, so a NaN score of a padded key row (its own row of the S^T tile, nobody else's) never reaches the softmax."""
    c = _mmdit_case("selector", T)
    X.check_output(c, _run_mmdit(X.pack_mmdit(c, engine_layout=True, k_pad=float("nan"))))


# ---- natinf_dit_attention_bf16 ------------------------------------------------------------------------------------------------------------------------------------

DIT_HD = [8, 16, 40, 56, 64, 72, 80, 88, 96]      # <2,4> at its smallest / largest widths, <3,5> at 72 / 80, <3,6> at 88 / 96: even and odd chunk counts, both sides of every dispatch boundary
DIT_FORMS = [(256, 0), (384, 0), (1024, 0), (256, RESIDENT)]
_form_id = lambda f: f"T{f[0]}_{'resident' if f[1] else 'streaming'}"


@functools.lru_cache(maxsize=8)
def _dit_case(family, T, hd):
    if family == "uniform":
        return X.uniform_case(2, max(2, -(-T // (2 * hd))), T, hd, seed=T + hd)
    return X.selector_case(2, 2, T, hd, seed=T + hd)


def _run_dit(p, flags):
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    buf, o = _dev(p["qkv"]), _dev(p["o"])
    base, D = ptr(buf), p["D"]
    check(lib.natinf_dit_attention_bf16(base, base + 2 * D, base + 4 * D, p["ld"], ptr(o), p["ld_o"], p["B"], p["T"], p["H"], p["hd"], flags, stream_ptr()),
          "natinf_dit_attention_bf16")
    torch.cuda.synchronize()
    return _host16(o)


@pytest.mark.parametrize("gapped", [False, True], ids=["engine_layout", "gapped"])
@pytest.mark.parametrize("form", DIT_FORMS, ids=_form_id)
@pytest.mark.parametrize("hd", DIT_HD)
def test_dit_attention_counts_every_key_exactly_once(hd, form, gapped):
    """uniform family on the engine's [B*T][3D] buffer, and with ld = 3D + 8 (finite gap columns) / ld_o = D + 4 (NaN canary in the output gap)"""
    T, flags = form
    c = _dit_case("uniform", T, hd)
    X.check_output(c, _run_dit(X.pack_dit(c, gapped=gapped), flags))


@pytest.mark.parametrize("gapped", [False, True], ids=["engine_layout", "gapped"])
@pytest.mark.parametrize("hd,form", [(hd, f) for hd in DIT_HD for f in DIT_FORMS if f[0] <= 2 ** hd], ids=lambda v: _form_id(v) if isinstance(v, tuple) else f"hd{v}")
def test_dit_attention_selects_the_permuted_value_row(hd, form, gapped):
    """selector family; head width 8 has 256 code words, so it runs at T = 256 only"""
    T, flags = form
    c = _dit_case("selector", T, hd)
    X.check_output(c, _run_dit(X.pack_dit(c, gapped=gapped), flags))


@pytest.mark.parametrize("hd", [8, 16, 40, 56, 80, 88])
def test_dit_attention_random_data_at_the_widths_no_other_test_launches(hd):
    """random data against an fp64 softmax at tests/test_gpu_dit512.py's bound, streaming (384 tokens: three query blocks, six key tiles) and resident"""
    B, H = 2, 2
    for T, flags in ((384, 0), (256, RESIDENT)):
        rng = np.random.default_rng(1000 * hd + T)
        z = lambda: X.bf16_bits(rng.standard_normal((B, T, H, hd)).astype(np.float32))
        p = X.pack_dit(X.Case("random", B, H, T, hd, z(), z(), z(), None))
        ref = X.bf16_f32(X.reference_dit(p)).astype(np.float64)
        out = X.bf16_f32(_run_dit(p, flags)).astype(np.float64)
        assert np.isfinite(out).all()
        err = np.abs(out - ref).max() / np.abs(ref).max()
        assert err <= ATTN_TOL, (T, flags, err)


@pytest.mark.parametrize("input_size", [32, 64])
@pytest.mark.parametrize("depth,hid,heads", [(2, 128, 4), (1, 640, 8)], ids=["hd32", "hd80"])
def test_dit_engine_at_head_widths_32_and_80_matches_oracle(depth, hid, heads, input_size):
    """the instantiations the kernel tests above cover for the first time (<2,4> below width 64, <3,5> at width 80) on the product path: one forward at 256 tokens
    (the LDS-resident kernel) and at 1,024 tokens (the streaming kernel) against oracle/dit_oracle.py"""
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.dit import DiTEngine, flatten_state_dict
    P = D.make_params(depth, hid, seed=7, grid=input_size // 2)
    g = torch.Generator().manual_seed(depth + hid + input_size)
    x, t, y = torch.randn(2, 4, input_size, input_size, generator=g), torch.tensor([900.0, 20.0]), torch.tensor([207, 1000])
    ref = D.forward(P, x, t, y, heads)
    eng = DiTEngine(flatten_state_dict(P, depth, hid), max_batch=2, depth=depth, hidden=hid, heads=heads, input_size=input_size)
    out = eng(x.cuda(), t.cuda(), y.cuda()).cpu()
    assert torch.isfinite(out).all()
    err = ((out - ref).abs().max() / ref.abs().max()).item()
    assert err <= TOL, err


# ---- the fp8 output epilogue (FlashArgs::o8 / omx) ------------------------------------------------------------------------------------------------------------------

def _run_fp8out(p):
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    assert "k" in p
    q, k, vT = _dev(p["q"]), _dev(p["k"]), _dev(p["vT"])
    B, H, Tp = p["B"], p["H"], p["Tp"]
    o8 = torch.full((B, Tp, 64 * H), 0xAA, dtype=torch.uint8, device="cuda")
    omx = torch.full((B, H // 2, Tp, 4), 0xAA, dtype=torch.uint8, device="cuda")
    check(lib.natinf_debug_attention_hd64_fp8out(ptr(q), ptr(k), p["ld_qk"], p["qk_bs"], ptr(vT), ptr(o8), ptr(omx), B, H, Tp, p["T"], 0.125, stream_ptr()),
          "natinf_debug_attention_hd64_fp8out")
    torch.cuda.synchronize()
    return o8.cpu().numpy(), omx.cpu().numpy()


@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("T", [129, 285])
def test_fp8_epilogue_exact_on_mx_exact_blocks(T, H, flash_mode):
    """selector family with V made of MX-exact blocks (attention_exact_cases.mx_exact_values): the 64 output bytes of row i, head h are the e4m3 codes of
    V[pi_h(i)], its two scale bytes are s + 127 at the documented positions, and every omx byte of the rows < T is accounted for."""
    B = 2
    vals, codes, sc = X.mx_exact_values(B, T, H, seed=T + H)
    c = X.selector_case(B, H, T, 64, seed=T + H, v=vals)
    o8, omx = _run_fp8out(X.pack_mmdit(c))
    Tp = omx.shape[2]
    want8 = np.empty((B, T, H, 64), np.uint8)
    wantmx = np.empty((B, H // 2, T, 4), np.uint8)
    for (b, h), perm in c.info["perms"].items():
        want8[b, :, h] = codes[b, perm, h]
        wantmx[b, h >> 1, :, (h & 1) * 2:(h & 1) * 2 + 2] = sc[b, perm, h]
    flat = omx.reshape(-1)                                                  # the documented index against the array view, at a few points
    for (b, h, t, blk) in ((0, 0, 0, 0), (1, H - 1, T - 1, 1), (1, 1, 64, 0)):
        assert flat[X.omx_index(b, h, t, blk, H, Tp)] == wantmx[b, h >> 1, t, (h & 1) * 2 + blk]
    bad = np.argwhere(omx[:, :, :T] != wantmx)
    assert not len(bad), (len(bad), bad[:4].tolist(), omx[:, :, :T][tuple(bad[0])], wantmx[tuple(bad[0])])
    got8 = o8[:, :T].reshape(B, T, H, 64)
    bad = np.argwhere(got8 != want8)
    assert not len(bad), (len(bad), bad[:4].tolist(), hex(got8[tuple(bad[0])]), hex(want8[tuple(bad[0])]))


def _bf16_ulp(x):
    x = np.abs(x)
    return np.where(x > 0, np.exp2(np.floor(np.log2(np.where(x > 0, x, 1.0))) - 7), 0.0)


@pytest.mark.parametrize("T,H", [(129, 2), (285, 4)])
def test_fp8_epilogue_random_data_against_the_bf16_output(T, H, flash_mode):
    """Random data, against natinf_attention_hd64_bf16 on the same operands and mode (the same accumulators x = O / l in fp32; the bf16 entry rounds them to o, at
    most half a bf16 ulp away).  Derived, not measured:
      scale: the written byte is the MX scale of the block's fp32 amax, which lies within half an ulp of the bf16 output's -- so it is the scale of SOME magnitude
             within one bf16 ulp of that (the scale is monotonic: between the scales of amax -+ ulp);
      value: |decoded - x| <= the e4m3 half-ulp at the written scale 2^e = max(2^-4 |x|, 2^(e-10)) (normal / subnormal codes; nothing saturates, the scale maps
             the block maximum to <= 448), and |x - o| <= ulp(o) / 2, so |decoded - o| <= max(2^-4 |o|, 2^(e-10)) + ulp(o)."""
    B = 2
    rng = np.random.default_rng(T + H)
    z = lambda s=1.0: X.bf16_bits((s * rng.standard_normal((B, T, H, 64))).astype(np.float32))
    p = X.pack_mmdit(X.Case("random", B, H, T, 64, z(2.0), z(), z(), None), v_pad=0.0)
    o = X.bf16_f32(_run_mmdit(p))[:, :T].astype(np.float64).reshape(B, T, H, 2, 32)
    assert np.isfinite(o).all()
    o8, omx = _run_fp8out(p)
    sc = np.empty((B, T, H, 2), np.int64)
    for h in range(H):
        sc[:, :, h] = omx[:, h >> 1, :T, (h & 1) * 2:(h & 1) * 2 + 2]
    amax = np.abs(o).max(axis=-1)
    ulp = _bf16_ulp(amax)
    lo, hi = X.mx_scale_byte(np.maximum(amax - ulp, 0.0)), X.mx_scale_byte(amax + ulp)
    assert ((sc >= lo) & (sc <= hi)).all(), np.argwhere((sc < lo) | (sc > hi))[:4].tolist()
    e = (sc - 127).astype(np.float64)[..., None]
    dec = X.e4m3_value(o8[:, :T].reshape(B, T, H, 2, 32)).astype(np.float64) * np.exp2(e)
    bound = np.maximum(2.0 ** -4 * np.abs(o), np.exp2(e - 10)) + _bf16_ulp(o)
    bad = np.argwhere(np.abs(dec - o) > bound)
    assert not len(bad), (len(bad), bad[:4].tolist())
