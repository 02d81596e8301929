"""The DiT engine's fp8 projections (NATINF_DIT_FP8, include/natinf_dit.h): per block the q | k | v, fc1 and fc2 GEMMs on e4m3 operands with fp32
accumulation -- per-output-channel weight scales, per-token scales out of the LayerNorm-modulate passes, E8M0 block scales between fc1 and fc2 -- everything
else bf16 as without the flag.  Five groups: the C ABI's contract, the K = 1,152 GEMMs alone against fp64 with a derived bound, the network against the fp32
oracle, the 24-step trajectory of the generation job, and the Python surface.

Measured bounds follow the convention of tests/test_gpu_accuracy.py's TOL_BY_LEVEL: the constant is 1.25 x the largest value observed on an MI355X over the
test's cases; measured value and bound are in the docstring of the test that uses them and in DESIGN.md section 4b."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

XL2 = dict(depth=28, hidden=1152, heads=16)
TOL_BF16 = 3e-2            # tests/test_gpu_dit.py: max |engine - oracle| / max |oracle| of the bf16 engine
# max |fp8 engine - oracle| / max |oracle|: 1.25 x the largest value observed over test_xl2_fp8_against_the_oracle (both stream widths) and
# test_small_configs_fp8 (all four cases): 2.045e-2 (DiT-XL/2, half stream)
TOL_FP8 = 2.56e-2
# measured fp8 / bf16 error ratio at DiT-XL/2 (test_xl2_fp8_against_the_oracle): 1.752e-2 / 3.559e-3 = 4.92 (fp32 stream), 2.045e-2 / 4.314e-3 = 4.74 (half stream)
FP8_OVER_BF16 = 4.92
# relative RMS difference of the fp8 job's final latents against the bf16 job's (test_trajectory_fp8_against_bf16): measured 2.260e-2
TOL_TRAJ_RMS = 2.83e-2


def _flat(P, depth, hid, S=32):
    from naturaldiffusion_amd.dit import flatten_state_dict
    return flatten_state_dict(P, depth, hid, S)


def _create(depth, hidden, heads, flags, size=None):
    from naturaldiffusion_amd._lib import lib
    h = C.c_void_p()
    rc = lib.natinf_dit_create(C.byref(h), depth, hidden, heads, flags) if size is None else lib.natinf_dit_create_sized(C.byref(h), depth, hidden, heads, size, flags)
    return rc, h


@pytest.fixture(scope="module")
def xl2_seed3():
    from oracle import dit_oracle as D
    P = D.make_params(28, 1152, seed=3)
    return P, _flat(P, 28, 1152)


@pytest.fixture(scope="module")
def xl2_synth():
    from naturaldiffusion_amd.synth import synthetic_dit_state_dict
    return _flat(synthetic_dit_state_dict(), 28, 1152)


# ------------------------------------------------------------------------------ 1. contract
@pytest.mark.parametrize("S", [32, 64])
@pytest.mark.parametrize("depth,hid,heads", [(2, 128, 2), (28, 1152, 16)])
def test_flag_creates_loads_and_runs(depth, hid, heads, S):
    from naturaldiffusion_amd._lib import DIT_FP8
    from naturaldiffusion_amd.dit import DiTEngine, FP8
    from naturaldiffusion_amd.synth import synthetic_dit_state_dict
    assert FP8 == DIT_FP8 == 2
    flat = _flat(synthetic_dit_state_dict(depth, hid, seed=1, input_size=S), depth, hid, S)
    eng = DiTEngine(flat, max_batch=2, depth=depth, hidden=hid, heads=heads, input_size=S, fp8=True)
    g = torch.Generator().manual_seed(S + depth)
    z = torch.randn(2, 4, S, S, generator=g).cuda()
    out = eng(z, torch.tensor([900.0, 20.0]).cuda(), torch.tensor([207, 1000]).cuda())
    torch.cuda.synchronize()
    assert out.shape == (2, 8, S, S) and torch.isfinite(out).all() and float(out.abs().max()) > 0
    assert torch.equal(out, eng(z, torch.tensor([900.0, 20.0]).cuda(), torch.tensor([207, 1000]).cuda())), "not run-to-run deterministic"


def test_create_time_rules():
    from naturaldiffusion_amd._lib import lib
    EINVAL = lib.natinf_dit_create(None, 1, 128, 2, 0)
    assert EINVAL != 0
    for hid, heads in ((576, 8), (192, 2)):                            # hidden % 128 != 0: refused, never a silent bf16 engine
        for flags in (2, 3):
            rc, _ = _create(1, hid, heads, flags)
            assert rc == EINVAL, (hid, flags, rc)
        rc, h = _create(1, hid, heads, 0)                              # (the same sizes are fine without the flag)
        assert rc == 0
        lib.natinf_dit_destroy(h)
    for flags in (4, 6, 7, 8, 1 << 20):                                # unknown flag bits
        for size in (None, 32, 64):
            rc, _ = _create(2, 128, 2, flags, size)
            assert rc == EINVAL, (flags, size, rc)
    for flags in (2, 3):                                               # with NATINF_DIT_UNFUSED_ATTENTION and both input sizes
        for size in (None, 32, 64):
            rc, h = _create(2, 128, 2, flags, size)
            assert rc == 0 and lib.natinf_dit_input_size(h) == (size or 32)
            lib.natinf_dit_destroy(h)
    from naturaldiffusion_amd.dit import DiTEngine
    with pytest.raises(ValueError):
        DiTEngine(torch.zeros(1), max_batch=1, depth=1, hidden=576, heads=8, fp8=True)


def test_packed_and_workspace_bytes_answer_for_the_mode():
    """The fp8 image holds qkv (3 D^2), fc1 (4 D^2) and fc2 (4 D^2) of every block as one byte per element instead of two, plus their per-output-channel
    fp32 scales (3 D + 4 D + D of them); everything else is packed as in the bf16 image.  The parameter vector is the same."""
    from naturaldiffusion_amd._lib import lib
    depth, D = XL2["depth"], XL2["hidden"]
    for flags in (0, 1):
        rc, hb = _create(depth, D, XL2["heads"], flags)
        rc8, h8 = _create(depth, D, XL2["heads"], flags | 2)
        assert rc == 0 and rc8 == 0
        assert lib.natinf_dit_param_count(hb) == lib.natinf_dit_param_count(h8)
        saved = depth * (11 * D * D * (2 - 1) - (3 * D + 4 * D + D) * 4)
        assert lib.natinf_dit_packed_bytes(hb) - lib.natinf_dit_packed_bytes(h8) == saved
        # workspace per sample: the bf16 GELU(fc1) buffer (T x 4 D x 2) is replaced by e4m3 rows of LN-modulate (T x D) and of GELU(fc1) (T x 4 D), the
        # per-token scales (T x 4) and the block scales (T x 4 D / 32)
        T = 256
        for B in (1, 16):
            assert lib.natinf_dit_workspace_bytes(hb, B) - lib.natinf_dit_workspace_bytes(h8, B) == B * (T * 4 * D * 2 - T * D - T * 4 * D - T * 4 - T * 4 * D // 32)
        lib.natinf_dit_destroy(hb)
        lib.natinf_dit_destroy(h8)


def _profile_of_a_forward(eng, n):
    from naturaldiffusion_amd._lib import lib, check
    g = torch.Generator().manual_seed(0)
    z, t, y = torch.randn(n, 4, 32, 32, generator=g).cuda(), torch.linspace(999.0, 3.0, n).cuda(), (torch.arange(n) * 60).cuda()
    eng(z, t, y)
    torch.cuda.synchronize()
    check(lib.natinf_gemm_profile(1), "natinf_gemm_profile")
    try:
        eng(z, t, y)
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 16)
        assert lib.natinf_gemm_profile_read(buf, len(buf)) > 0
    finally:
        lib.natinf_gemm_profile(0)
    rows = {}
    for line in buf.value.decode().splitlines():
        f = line.split()
        rows[(int(f[0]), int(f[1]), int(f[2]), f[6])] = int(f[7])
    return rows


def test_profile_lists_the_fp8_kernels(xl2_synth):
    from naturaldiffusion_amd.dit import DiTEngine
    eng = DiTEngine(xl2_synth, max_batch=16, fp8=True, **XL2)
    rows = _profile_of_a_forward(eng, 16)
    print(rows)
    fp8 = {k: v for k, v in rows.items() if "fp8" in k[3]}
    for (M, N, K), epi, mxa in (((4096, 3456, 1152), "/e1", False), ((4096, 4608, 1152), "/e2", False), ((4096, 1152, 4608), "/e3", True)):
        hit = [(k, v) for k, v in fp8.items() if k[:3] == (M, N, K)]
        assert len(hit) == 1 and hit[0][1] == 28, (M, N, K, hit)
        assert hit[0][0][3].endswith(epi) and ("_mxa" in hit[0][0][3]) == mxa, hit
    assert sum(fp8.values()) == 3 * 28
    assert any(k[:3] == (4096, 1152, 1152) and "fp8" not in k[3] and v == 28 for k, v in rows.items())       # the attention output projection stays bf16
    del eng
    bf = _profile_of_a_forward(DiTEngine(xl2_synth, max_batch=16, **XL2), 16)                              # created afterwards, same process
    assert bf and not any("fp8" in k[3] for k in bf)


# ------------------------------------------------------------------------------ 2. the GEMM alone, exact bound
def _ulp(x, mant_bits):
    """spacing of a binary format with ``mant_bits`` stored mantissa bits at |x| (normal range)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-300))) - mant_bits)


@pytest.mark.parametrize("M,N,K,epi", [(4096, 3456, 1152, "bf16"), (4096, 1152, 1152, "bf16"), (4096, 1152, 1152, "f32"), (4096, 4608, 1152, "gelu_mx"),
                                       (4000, 3456, 1152, "bf16"), (4000, 4608, 1152, "gelu_mx"), (264, 1152, 384, "bf16")])
def test_k1152_gemm_against_fp64(M, N, K, epi):
    """DiT-XL/2's three K = 1,152 GEMM shapes (nine 128-byte K-tiles) with the epilogues the engine runs on them -- q | k | v: scales + bias -> bf16; fc1: scales + bias +
    tanh-GELU -> e4m3 + E8M0 block scales -- plus N = 1,152 (4.5 tile columns) with the bf16 and the fp32 output, an M that is no multiple of 256, and three K-tiles
    (the shortest odd count).  One tile: w128_fp8_ok() keeps the four-wave kernel to even K-tile counts (its odd-count form was measured level with the eight-wave
    tile and not kept), so these shapes run on k_gemm_fp8 whatever natinf_set_gemm_w128 says.

    Reference: fp64 on the DEQUANTISED operands.  e4m3 values times power-of-two-free fp32 scales are exact in fp64 and so is every product (4 + 24 + 4 + 24 bits),
    so the kernel differs from it by its fp32 accumulation -- |sum error| <= K * 2^-24 * sum_k |a_k b_k| (K additions, each rounding error at most 2^-24 of a
    partial sum that sum_k |a_k b_k| bounds; the three epilogue roundings, two scale products and the bias, are covered by the same term since K >= 384) -- and by
    the rounding to the output type: one ulp of it at the reference value.  For the GELU epilogue the accumulation term passes through GELU (slope <= 1.13) and the
    kernel's tanh (hardware exp2 and rcp, 1 ulp each, on an argument below 2^5) adds at most 2^-21 (|x| + |GELU(x)|); the e4m3 ulp is taken at the block scale
    the KERNEL wrote (the value's binade, not below the subnormal step 2^-9 of the scale)."""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.randn(M, K, generator=g) * (torch.rand(M, 1, generator=g) * 3 + 0.1)).cuda()
    b = (torch.randn(N, K, generator=g) * 0.05).cuda()
    bias = torch.randn(N, generator=g).cuda()
    qa, sa = torch.empty(M, K, dtype=torch.uint8, device="cuda"), torch.empty(M, device="cuda")
    qb, sb = torch.empty(N, K, dtype=torch.uint8, device="cuda"), torch.empty(N, device="cuda")
    check(lib.natinf_debug_quant_fp8_rows(ptr(a), ptr(qa), ptr(sa), M, K, stream_ptr()), "quant")
    check(lib.natinf_debug_quant_fp8_rows(ptr(b), ptr(qb), ptr(sb), N, K, stream_ptr()), "quant")
    da = qa.view(torch.float8_e4m3fn).double() * sa.double()[:, None]
    db = qb.view(torch.float8_e4m3fn).double() * sb.double()[:, None]
    x = da @ db.t() + bias.double()
    acc = K * 2.0 ** -24 * (da.abs() @ db.abs().t() + bias.double().abs())
    if epi == "bf16":
        c = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        check(lib.natinf_debug_gemm_fp8(M, N, K, ptr(qa), ptr(sa), None, ptr(qb), ptr(sb), ptr(bias), ptr(c), None, 0, 1, stream_ptr()), "gemm_fp8")
        err, bound = (c.double() - x).abs(), acc + _ulp(x, 7)
    elif epi == "f32":
        c = torch.empty(M, N, device="cuda")
        check(lib.natinf_debug_gemm_fp8(M, N, K, ptr(qa), ptr(sa), None, ptr(qb), ptr(sb), ptr(bias), ptr(c), None, 1, 1, stream_ptr()), "gemm_fp8")
        err, bound = (c.double() - x).abs(), acc + _ulp(x, 23)
    else:
        c8, cmt = torch.empty(M, N, dtype=torch.uint8, device="cuda"), torch.empty((N // 128) * M * 4, dtype=torch.uint8, device="cuda")
        check(lib.natinf_debug_gemm_fp8(M, N, K, ptr(qa), ptr(sa), None, ptr(qb), ptr(sb), ptr(bias), ptr(c8), ptr(cmt), 3 | (2 << 8), 1, stream_ptr()), "gemm_fp8")
        cm = cmt.reshape(N // 128, M, 4).permute(1, 0, 2).reshape(M, N // 32)                                  # K-tile-major planes -> [M][N / 32]
        s = torch.exp2(cm.double() - 127)[..., None].expand(M, N // 32, 32).reshape(M, N)
        got = c8.view(torch.float8_e4m3fn).double() * s
        ref = torch.nn.functional.gelu(x, approximate="tanh")
        ulp8 = s * torch.exp2(torch.floor(torch.log2((ref.abs() / s).clamp_min(2.0 ** -6))) - 3)
        err, bound = (got - ref).abs(), 1.13 * acc + 2.0 ** -21 * (x.abs() + ref.abs()) + ulp8
        # (the kernel's own fp32 value fits its block scale, |v| <= 448 s; the reference is at most the accumulation term away from it)
        assert (ref.abs() <= 448 * s + 1.13 * acc + 2.0 ** -21 * (x.abs() + ref.abs())).all(), "a block scale too small for its block"
    torch.cuda.synchronize()
    worst = float((err / bound).max())
    print(f"fp8 GEMM ({M}, {N}, {K}) {epi}: max err / bound {worst:.3f}, max rel err {float(err.max() / x.abs().max()):.3e}")
    assert torch.isfinite(err).all() and worst <= 1.0, worst


# ------------------------------------------------------------------------------ 3. network accuracy
def _rel(out, ref):
    return float(np.abs(out - ref).max() / np.abs(ref).max())


def test_xl2_fp8_against_the_oracle(xl2_seed3):
    """tests/test_gpu_dit.py::test_xl2_matches_oracle_and_batch_independent's inputs (seed-3 weights, three samples) on the fp8 engine next to the bf16 engine, under
    both residual-stream widths.  Measured on an MI355X, max |engine - oracle| / max |oracle|: fp32 stream bf16 3.559e-3 / fp8 1.752e-2 (ratio 4.92); half stream
    bf16 4.314e-3 / fp8 2.045e-2 (ratio 4.74) -- the MMDiT pair sits at ~5.  TOL_FP8 = 2.56e-2 = 1.25 x the largest fp8 figure of this file's network cases
    (2.045e-2, here).
    Batch independence: sample 2 in a batch of three and as row 0 of a batch of 8 agree to the bf16 test's 1e-2 of max |oracle| scaled by the measured ratio,
    4.92e-2 (measured: 0.0, identical bytes -- a row of a GEMM and a token's scale see nothing of the other samples, and a sum over K runs in the same order on
    whichever tile the row count selects)."""
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.dit import DiTEngine
    P, flat = xl2_seed3
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 4, 32, 32, generator=g)
    t = torch.tensor([999.0, 500.0, 3.0])
    y = torch.tensor([1000, 207, 0])
    ref = D.forward(P, x, t, y, 16).numpy()
    xb = torch.cat([x[2:3], torch.randn(5, 4, 32, 32, generator=g)]).cuda()
    tb = torch.cat([t[2:3], torch.full((5,), 77.0)]).cuda()
    yb = torch.cat([y[2:3], torch.tensor([3, 4, 5, 6, 7])]).cuda()
    for s16 in (False, True):
        errs = {}
        for fp8 in (False, True):
            eng = DiTEngine(flat, max_batch=8, stream16=s16, fp8=fp8)
            out = eng(x.cuda(), t.cuda(), y.cuda()).cpu().numpy()
            errs[fp8] = _rel(out, ref)
            if fp8:
                out8 = eng(xb, tb, yb).cpu().numpy()
                indep = float(np.abs(out8[0] - out[2]).max() / np.abs(ref).max())
            del eng
        print(f"DiT-XL/2 stream16={s16}: max rel err against the oracle bf16 {errs[False]:.3e}, fp8 {errs[True]:.3e} (ratio {errs[True] / errs[False]:.2f}); "
              f"fp8 sample 2 alone vs row 0 of 8: {indep:.3e}")
        assert errs[False] <= TOL_BF16, (s16, errs)
        assert errs[True] <= TOL_FP8, (s16, errs)
        assert indep <= 1e-2 * FP8_OVER_BF16, (s16, indep)


def test_workspace_state_does_not_reach_the_output(xl2_seed3):
    """A forward on a workspace pre-filled with finite garbage -- 3.0e4 as fp32, bf16 and IEEE half, and the byte 0x7e (448 as e4m3, 2^-1 as E8M0) -- gives the
    bytes of a forward on a zeroed workspace: every fp8 / MX operand row a kernel reads was written by the same forward (M = B x 256 is whole row tiles)."""
    from naturaldiffusion_amd.dit import DiTEngine
    _, flat = xl2_seed3
    g = torch.Generator().manual_seed(6)
    for n, unfused in ((3, False), (5, True)):
        eng = DiTEngine(flat, max_batch=8, fp8=True, unfused_attention=unfused)
        z, t, y = torch.randn(n, 4, 32, 32, generator=g).cuda(), torch.linspace(900.0, 5.0, n).cuda(), torch.arange(n).cuda() * 100
        eng._ws.zero_()
        want = eng(z, t, y).clone()
        assert torch.isfinite(want).all()
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            eng._ws.view(dt).fill_(3.0e4)
            assert torch.equal(eng(z, t, y), want), (unfused, dt)
        eng._ws.fill_(0x7e)
        assert torch.equal(eng(z, t, y), want), (unfused, "0x7e")
        del eng


@pytest.mark.parametrize("unfused", [False, True])
@pytest.mark.parametrize("tag,depth,hid,heads", [("s64", 2, 128, 2), ("h1152", 1, 1152, 16)])
def test_small_configs_fp8(golden_dir, tag, depth, hid, heads, unfused):
    """tests/golden/dit_forward.npz's s64 case (hidden 128: one K-tile, the eight-wave tile) and hidden 1,152 / depth 1 / 16 heads (head dim 72, nine K-tiles) against
    oracle.dit_oracle.forward, fused and per-head attention.  Measured, fp8 (bf16 beside it): s64 8.644e-3 (2.743e-3), fused and per head alike; h1152 3.923e-3
    (2.408e-3), alike; bound TOL_FP8 = 2.56e-2."""
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.dit import DiTEngine
    P = D.make_params(depth, hid, seed=7)
    if tag == "s64":
        fx = np.load(golden_dir / "dit_forward.npz")
        x, t, y = (torch.from_numpy(fx[f"{tag}_{k}"]) for k in ("x", "t", "y"))
    else:
        g = torch.Generator().manual_seed(72)
        x, t, y = torch.randn(3, 4, 32, 32, generator=g), torch.tensor([950.0, 410.0, 8.0]), torch.tensor([17, 1000, 999])
    ref = D.forward(P, x, t, y, heads).numpy()
    if tag == "s64":
        assert np.allclose(ref, fx["s64_out"], rtol=1e-4, atol=1e-5)
    errs = {}
    for fp8 in (False, True):
        eng = DiTEngine(_flat(P, depth, hid), max_batch=4, depth=depth, hidden=hid, heads=heads, unfused_attention=unfused, fp8=fp8)
        errs[fp8] = _rel(eng(x.cuda(), t.cuda(), y.cuda()).cpu().numpy(), ref)
    print(f"DiT {tag} unfused={unfused}: max rel err against the oracle bf16 {errs[False]:.3e}, fp8 {errs[True]:.3e}")
    assert errs[False] <= TOL_BF16 and errs[True] <= TOL_FP8, errs


# ------------------------------------------------------------------------------ 4. trajectory
def test_trajectory_fp8_against_bf16(xl2_synth):
    """generate_sharded(16, ddim, 24 steps, batch 16, seed 0) on DiT-XL/2 with synthetic weights: relative RMS difference of the fp8 job's final latents against
    the bf16 job's -- measured 2.260e-2, bound TOL_TRAJ_RMS = 2.83e-2 (1.25 x) -- and the fp8 job's images as identical bytes under a world=2 split and at batch
    size 8 (forwards of 16 samples instead of 32): the noise is counter-based by global index, and neither the per-token scales nor the kernels a forward of
    another size takes couple or re-order a sample's arithmetic."""
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd.dit import DiTEngine
    kw = dict(alg_name="ddim", num_step=24, seed=0, decode=False)
    bf = DiTEngine(xl2_synth, max_batch=32, **XL2)
    zb, _, ib, _ = V.generate_sharded(16, batch_size=16, model=bf, **kw)
    del bf
    eng = DiTEngine(xl2_synth, max_batch=32, fp8=True, **XL2)
    z8, _, i8, _ = V.generate_sharded(16, batch_size=16, model=eng, fp8=True, **kw)
    assert torch.isfinite(z8).all() and i8.tolist() == ib.tolist() == list(range(16))
    rms = float(((z8 - zb).double().pow(2).mean() / zb.double().pow(2).mean()).sqrt())
    print(f"fp8 vs bf16 job, 24 ddim steps, final latents: relative RMS difference {rms:.3e}")
    assert rms <= TOL_TRAJ_RMS, rms
    half, _, ih, _ = V.generate_sharded(16, batch_size=8, model=eng, fp8=True, **kw)
    assert ih.tolist() == list(range(16)) and torch.equal(half, z8), "batch size 8 vs 16"
    for r in range(2):
        z, _, ix, _ = V.generate_sharded(16, batch_size=16, rank=r, world=2, model=eng, fp8=True, **kw)
        assert ix.tolist() == list(range(r, 16, 2)) and torch.equal(z, z8[ix.to(z8.device)]), f"rank {r} of 2"
    with pytest.raises(ValueError):                                     # fp8=True never runs quietly on a bf16 engine
        V.generate_sharded(2, batch_size=2, model=DiTEngine(xl2_synth, max_batch=4, **XL2), fp8=True, **kw)


# ------------------------------------------------------------------------------ 5. the Python surface
def test_load_dit_engine_keeps_the_two_modes_apart(tmp_path, monkeypatch):
    from oracle import dit_oracle as D
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd import dit
    P = D.make_params(1, 128, seed=2)
    path = tmp_path / "dit.pt"
    torch.save({k: v.clone() for k, v in P.items()}, path)
    monkeypatch.setattr(dit, "XL2", dict(depth=1, hidden=128, heads=2))
    monkeypatch.setattr(V, "device", "cuda:0")
    a = V.load_dit_engine(path, max_batch=2)
    b = V.load_dit_engine(path, max_batch=2, fp8=True)
    assert a is not b and not a.fp8 and b.fp8
    assert V.load_dit_engine(path, max_batch=2, fp8=True) is b and V.load_dit_engine(path, max_batch=2) is a
    g = torch.Generator().manual_seed(1)
    z = torch.randn(2, 4, 32, 32, generator=g).cuda()
    oa, ob = a(z, torch.tensor([5.0, 700.0]).cuda(), torch.tensor([1, 2]).cuda()), b(z, torch.tensor([5.0, 700.0]).cuda(), torch.tensor([1, 2]).cuda())
    assert not torch.equal(oa, ob) and float((oa - ob).abs().max() / oa.abs().max()) <= TOL_FP8 + TOL_BF16
