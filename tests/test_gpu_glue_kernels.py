"""The glue kernels at the two ends of the DiT, SD3-MMDiT and AutoencoderKL engines ALONE against fp64 (tests/glue_kernel_cases.py: cases, references, radii and
comparators; their attainability and the mutants they catch: tests/test_glue_kernels_host.py): k_patch_embed<XH, GUARD> and the load-time k_transpose_f32 through
natinf_debug_patch_embed, k_dit_time_freq, k_dit_cond, k_silu_bf16, k_f32_to_bf16, k_unpatchify through their natinf_debug_* entries (include/natinf_dit.h),
k_vae_latents, k_vae_images and k_vae_quant through theirs (include/natinf_vae.h) -- the engines' own launchers and grids.  Every output sits between canaries that
must come back untouched; no case and no element is left out of a comparison.  Each test prints its worst (|value - reference| - half an output ulp) / radius.

Worst figures measured on an MI355X (a figure of 1 would be the edge of the radius; 0.000 means `below the output's rounding`): patch embedding 0.000 on all 48 shape /
stream pairs, plain and guarded (integer inputs: exact), beyond the half range inf unguarded and 65,504 with 27 counts of 27 guarded; time embedding 0.119 (B = 3, 7 and 4,100);
cond 0.241 (D 1152, B 920), 0.000 at B = 3; SiLU 0.000; k_vae_latents 0.000; k_vae_quant 0.502 (N 2, hw 63).  The part of an error that neither the output's rounding nor the
analytic radius explains -- what the device functions' allowances are for -- is 0.000 in every transcendental case.  All 98 tests pass: no defect in a kernel, no kernel changed."""
import ctypes as C

import numpy as np
import pytest
import torch

import glue_kernel_cases as G

pytestmark = pytest.mark.gpu

PAD = 64                                                                    # canary elements before and after a flat output


def _dev(a):
    a = np.array(a, order="C")                                              # a copy: the cases are shared and read-only
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(view)).cuda()


def _api():
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    return lib, check, ptr, stream_ptr


def _bf16_out(n):
    return torch.full((PAD + n + PAD,), G.BF16_CANARY, dtype=torch.int16, device="cuda")


def _bf16_back(buf, n, what):
    torch.cuda.synchronize()
    out = buf.cpu().numpy().view(np.uint16)
    assert np.all(out[:PAD] == G.BF16_CANARY) and np.all(out[PAD + n:] == G.BF16_CANARY), f"a canary around {what} was written"
    return out[PAD:PAD + n]


def _f32_out(n):
    return torch.full((PAD + n + PAD,), float("nan"), dtype=torch.float32, device="cuda")


def _f32_back(buf, n, what):
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.all(np.isnan(out[:PAD])) and np.all(np.isnan(out[PAD + n:])), f"a canary around {what} was written"
    return out[PAD:PAD + n]


def _patch_call(c, half, guarded):
    """one natinf_debug_patch_embed call; returns (x with its canary rows, the transpose scratch with its canaries, the guard's two words or None)"""
    lib, check, ptr, stream_ptr = _api()
    rows, D, K = c["rows"], c["D"], c["K"]
    z, w, bias, pos = _dev(c["z"]), _dev(c["w"]), _dev(c["bias"]), _dev(c["pos"])
    wt = torch.full((1 + K * D + 1,), float("nan"), dtype=torch.float32, device="cuda")
    x = torch.full((rows + 2, D), float("nan"), dtype=torch.float16 if half else torch.float32, device="cuda")
    slot = torch.tensor([-1, -1, 0, 0, -1, -1], dtype=torch.int32, device="cuda") if guarded else None      # {max_bits, count} zeroed between 0xffffffff words
    check(lib.natinf_debug_patch_embed(ptr(z), ptr(w), ptr(wt) + 4, ptr(bias), ptr(pos), ptr(x) + D * (2 if half else 4), int(half), ptr(slot) + 8 if guarded else None,
                                       c["C"], c["g"], D, c["B"], stream_ptr()), "natinf_debug_patch_embed")
    torch.cuda.synchronize()
    xs = x.cpu().numpy()
    if half:
        xs = xs.view(np.uint16)
    words = None
    if guarded:
        sw = slot.cpu().numpy().view(np.uint32)
        assert np.all(sw[[0, 1, 4, 5]] == 0xffffffff), "a word beside the guard slot was written"
        words = sw[2:4]
    return xs, wt.cpu().numpy(), words


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("C_,g,B,D", G.patch_case_ids(), ids=lambda v: str(v))
def test_patch_embed(C_, g, B, D, half):
    """k_patch_embed<half, false> then <half, true> on one case: within the radius, the transpose scratch equal to w^T in bytes, the guarded bytes equal to the plain
    bytes, the slot's count 0 and its maximum the bit pattern of the largest |value| before rounding"""
    c = G.patch_case(C_, g, B, D)
    x, wt, _ = _patch_call(c, half, False)
    fails, ratio = G.check_patch(c, half, x, wt)
    xg, wtg, slot = _patch_call(c, half, True)
    fails_g, ratio_g = G.check_patch(c, half, xg, wtg, slot, plain=x)
    print(f"\npatch_embed {c['name']} {'f16' if half else 'f32'}: worst (|x - y| - half ulp) / delta = {max(ratio, ratio_g):.3f}; guard max {slot[0]:#x} count {slot[1]}")
    assert not fails, fails
    assert not fails_g, fails_g


def test_patch_embed_beyond_the_half_range():
    """the half stream with a bias of 7e4 on one channel: the bare cast gives IEEE inf, the guarded form +-65,504 with one count per such element (the guard's stated
    contract, csrc/ncsnpp_kernels.h); every other channel as usual"""
    c = G.patch_case(*G.OVERFLOW_CASE, overflow=True)
    x, wt, _ = _patch_call(c, True, False)
    fails, _ = G.check_patch(c, True, x, wt)
    xg, wtg, slot = _patch_call(c, True, True)
    fails_g, _ = G.check_patch(c, True, xg, wtg, slot)
    print(f"\npatch_embed {c['name']}: unguarded channel {G.OVERFLOW_CH} = {x[1, G.OVERFLOW_CH]:#x}, guarded = {xg[1, G.OVERFLOW_CH]:#x}, count {slot[1]} of {c['rows']} rows")
    assert not fails, fails
    assert not fails_g, fails_g


@pytest.mark.parametrize("B", G.TIME_B)
def test_dit_time_freq(B):
    lib, check, ptr, stream_ptr = _api()
    c = G.time_case(B)
    emb = _bf16_out(B * 256)
    t = _dev(c["t"])
    check(lib.natinf_debug_dit_time_freq(ptr(t), ptr(emb) + 2 * PAD, B, stream_ptr()), "natinf_debug_dit_time_freq")
    k = G.bf16_bits_to_f64(_bf16_back(emb, B * 256, "emb")).reshape(B, 256)
    bad, ratio = G.check_interval(c["y"], c["delta"], k, "bf16")
    ana = G.time_case(B, dev=False)["delta"]
    unexplained = float(np.max(np.maximum(np.abs(k - c["y"]) - G.half_ulp_bf16(k) - ana, 0.0) / np.maximum(c["delta"] - ana, 1e-300)))
    print(f"\ndit_time_freq B {B}: worst (|emb - y| - half ulp) / delta = {ratio:.3f}; worst part the analytic radius does not explain / device allowance = {unexplained:.3f}")
    assert not bad, [(i // 256, i % 256) for i in bad[:8]]


@pytest.mark.parametrize("D,B", [(D, G.COND_B) for D in G.COND_D] + [G.COND_LARGE])
def test_dit_cond(D, B):
    lib, check, ptr, stream_ptr = _api()
    c = G.cond_case(D, B)
    n = c["B"] * D
    cs = _bf16_out(n)
    c0, table, y = _dev(c["c0"]), _dev(c["table"]), _dev(c["labels"])
    check(lib.natinf_debug_dit_cond(ptr(c0), ptr(table), ptr(y), ptr(cs) + 2 * PAD, D, c["B"], stream_ptr()), "natinf_debug_dit_cond")
    k = G.bf16_bits_to_f64(_bf16_back(cs, n, "cs")).reshape(c["B"], D)
    bad, ratio = G.check_interval(c["y"], c["delta"], k, "bf16")
    ana = G.cond_case(D, B, dev=False)["delta"]
    unexplained = float(np.max(np.maximum(np.abs(k - c["y"]) - G.half_ulp_bf16(k) - ana, 0.0) / np.maximum(c["delta"] - ana, 1e-300)))
    print(f"\ndit_cond D {D} B {B}: worst (|cs - y| - half ulp) / delta = {ratio:.3f}; unexplained / device allowance = {unexplained:.3f}")
    assert not bad, [(i // D, i % D) for i in bad[:8]]


@pytest.mark.parametrize("n", G.SILU_N)
def test_silu_bf16(n):
    lib, check, ptr, stream_ptr = _api()
    c = G.silu_case(n)
    cs = _bf16_out(n)
    x = _dev(c["x"])
    check(lib.natinf_debug_silu_bf16(ptr(x), ptr(cs) + 2 * PAD, n, stream_ptr()), "natinf_debug_silu_bf16")
    k = G.bf16_bits_to_f64(_bf16_back(cs, n, "cs"))
    bad, ratio = G.check_interval(c["y"], c["delta"], k, "bf16")
    ana = G.silu_case(n, dev=False)["delta"]
    unexplained = float(np.max(np.maximum(np.abs(k - c["y"]) - G.half_ulp_bf16(k) - ana, 0.0) / np.maximum(c["delta"] - ana, 1e-300)))
    print(f"\nsilu_bf16 n {n}: worst (|cs - y| - half ulp) / delta = {ratio:.3f}; unexplained / device allowance = {unexplained:.3f}")
    assert not bad, [(i, float(c["x"][i])) for i in bad[:8]]


@pytest.mark.parametrize("n", G.CAST_N)
def test_f32_to_bf16(n):
    """bytes: round to nearest even, ties both ways, -0.0, bf16 sub-normals, the largest finite fp32 to inf, a NaN stays a NaN"""
    lib, check, ptr, stream_ptr = _api()
    c = G.cast_case(n)
    dst = _bf16_out(n)
    x = _dev(c["x"])
    check(lib.natinf_debug_f32_to_bf16(ptr(x), ptr(dst) + 2 * PAD, n, stream_ptr()), "natinf_debug_f32_to_bf16")
    got = _bf16_back(dst, n, "dst")
    bad = G.check_bf16_bytes(c["bits"], got, c["nan"])
    assert not bad, [(i, hex(int(c["x"].view(np.uint32)[i])), hex(int(got[i])), hex(int(c["bits"][i]))) for i in bad[:8]]


@pytest.mark.parametrize("g", G.UNPATCH_G)
@pytest.mark.parametrize("OC", G.UNPATCH_OC)
def test_unpatchify(OC, g):
    """bytes: the tokens hold their own index, so any wrong permutation shows"""
    lib, check, ptr, stream_ptr = _api()
    c = G.unpatch_case(OC, g)
    n = c["out"].size
    out = _f32_out(n)
    tok = _dev(c["tok"])
    check(lib.natinf_debug_unpatchify(ptr(tok), ptr(out) + 4 * PAD, OC, g, c["N"], stream_ptr()), "natinf_debug_unpatchify")
    got = _f32_back(out, n, "out")
    assert np.array_equal(got.view(np.uint32), c["out"].ravel().view(np.uint32))


@pytest.mark.parametrize("R_", G.IMAGES_R)
def test_vae_images(R_):
    """bytes: bf16 of the picture in channels 0..2 of the interior (an interior -0.0 keeps its sign, a NaN stays a NaN), +0 bits on the border and in channels >= 3"""
    lib, check, ptr, stream_ptr = _api()
    c = G.images_case(R_)
    n = c["bits"].size
    y = _bf16_out(n)                                                        # (PAD * 2 bytes = 128: the output stays 16-byte aligned)
    img = _dev(c["img"])
    check(lib.natinf_debug_vae_images(ptr(img), ptr(y) + 2 * PAD, R_, G.VAE_B, stream_ptr()), "natinf_debug_vae_images")
    bad = G.check_bf16_bytes(c["bits"], _bf16_back(y, n, "y"), c["nan"])
    assert not bad, bad[:8]


@pytest.mark.parametrize("r_", G.LATENTS_R)
@pytest.mark.parametrize("C_", G.LATENTS_C)
def test_vae_latents(C_, r_):
    lib, check, ptr, stream_ptr = _api()
    c = G.latents_case(C_, r_)
    n = c["y"].size
    y = _bf16_out(n)
    z, W, bias = _dev(c["z"]), _dev(c["W"]), _dev(c["bias"])
    check(lib.natinf_debug_vae_latents(ptr(z), ptr(W), ptr(bias), ptr(y) + 2 * PAD, C_, r_, G.VAE_B, stream_ptr()), "natinf_debug_vae_latents")
    fails, ratio = G.check_latents(c, _bf16_back(y, n, "y"))
    print(f"\nvae_latents C {C_} r {r_}: worst (|y16 - y| - half ulp) / delta = {ratio:.3f}")
    assert not fails, fails


@pytest.mark.parametrize("hw", G.QUANT_HW)
@pytest.mark.parametrize("N", G.QUANT_N)
def test_vae_quant(N, hw):
    lib, check, ptr, stream_ptr = _api()
    c = G.quant_case(N, hw)
    n = c["y"].size
    out = _f32_out(n)
    m, W, bias = _dev(c["m"]), _dev(c["W"]), _dev(c["bias"])
    check(lib.natinf_debug_vae_quant(ptr(m), ptr(W), ptr(bias), ptr(out) + 4 * PAD, N, hw, G.VAE_B, stream_ptr()), "natinf_debug_vae_quant")
    bad, ratio = G.check_interval(c["y"], c["delta"], _f32_back(out, n, "out").reshape(c["y"].shape), "f32")
    print(f"\nvae_quant N {N} hw {hw}: worst |out - y| / delta = {ratio:.3f}")
    assert not bad, bad[:8]
