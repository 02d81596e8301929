"""GPU tests of the x0 correction of the CIFAR10 form (include/natinf.h: natinf_x0_threshold_f64, natinf_step_f64hist_x0fix): the predicted x0
of every image is clipped or dynamically thresholded, inside the step's launch, before the history and the sum see it.  Every comparison is byte
equality: the correction against the numpy mirror (sampler.x0_threshold_host, itself pinned to the reference and to torch by
tests/test_x0_threshold_host.py), the fused step against existing entries run one after the other on a copy of the slab."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from naturaldiffusion_amd import coeffgen as G
from naturaldiffusion_amd.coeff import load_coeff_npz
from oracle import ni_oracle as O

SEED = 888
COL0 = 2 ** 31
FIRST, STRIDE = 11, 3
N_IMG = 3
SIZES = [3072, 4, 8, 260, 8192]            # 32x32x3; one quad; two; 65 quads (a ragged last wave); the cap (the 64 KB instantiation)
CASES = [("clip", 0.995, 1.0), ("dynamic", 0.995, 1.0), ("dynamic", 0.5, 0.5), ("dynamic", 0.0, 1.0), ("dynamic", 1.0, 1.0)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def matrices(repo_root):
    return {"det5": load_coeff_npz(repo_root / "weights/step_5_weight_00.npz"), "sde5": G.vp_euler(5, stochastic=True)}


def kinds(n, seed):
    """the fixture's kinds of rows (tests/golden/make_golden_x0_threshold.py) at any size: ties, zeros, a NaN, two infinities, |x| under 1
    (max_val decides), |x| far over 1 (the quantile decides) -> fp64 [6, n]"""
    rs = np.random.RandomState(seed)
    x = np.zeros((6, n))
    x[0] = rs.randint(-6, 7, size=n) / 4.0
    x[2] = rs.randn(n)
    x[2, rs.randint(n)] = np.nan
    x[3] = rs.randn(n)
    x[3, 0], x[3, n - 1] = np.inf, -np.inf
    x[4] = rs.randn(n) * 0.25
    x[5] = rs.randn(n) * 2.0
    return x


def same_bytes(t, a):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------------------------ 1. the correction on its own
@pytest.mark.parametrize("epi", SIZES)
def test_threshold_entry_equals_the_mirror(dev, epi):
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr, X0_CLIP, X0_DYNAMIC
    from naturaldiffusion_amd.sampler import x0_threshold_host
    x = kinds(epi, 7 + epi)
    decided_by = set()
    for mode, ratio, max_val in CASES + [("dynamic", 0.995, 0.5), ("clip", 0.0, 0.5)]:
        want, s = x0_threshold_host(x, mode, ratio, max_val)
        buf = torch.from_numpy(x.copy()).to(dev)
        s_out = torch.full((6,), -7.0, dtype=torch.float64, device=dev)
        code = X0_CLIP if mode == "clip" else X0_DYNAMIC
        assert lib.natinf_x0_threshold_f64(ptr(buf), ptr(s_out), 6, epi, code, ratio, max_val, stream_ptr()) == 0
        assert same_bytes(s_out, s), (mode, ratio, max_val, s_out.cpu().numpy(), s)
        assert same_bytes(buf, want), (mode, ratio, max_val)
        if mode == "dynamic":
            decided_by |= {"max_val" if v == max_val else "quantile" for v in s[[0, 4, 5]]}
            assert np.isnan(s[2]) and s[1] == max_val
    assert decided_by == {"max_val", "quantile"}
    # s_out is optional
    buf = torch.from_numpy(x.copy()).to(dev)
    assert lib.natinf_x0_threshold_f64(ptr(buf), None, 6, epi, X0_DYNAMIC, 0.995, 1.0, stream_ptr()) == 0
    assert same_bytes(buf, x0_threshold_host(x, "dynamic", 0.995, 1.0)[0])


# ------------------------------------------------------------------------------ 2. the fused step
def raw_noise_step(ni, k, x, out, noise, hist, xn, epi, n_terms=None, c_diag=None):
    """natinf_step_f64hist_noise on the slab `hist` with ni's rows (a deterministic matrix: its one-term noise row); n_terms / c_diag override
    the signal row"""
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    idx, val, n = ni.rows.ptrs(k)
    ib, vb, nb = ni._noise_rows().ptrs(k)
    return lib.natinf_step_f64hist_noise(ptr(x), ptr(out), ptr(noise), ptr(hist), ptr(xn), idx, val, n if n_terms is None else n_terms,
                                         ni.rows.rows[k].diag if c_diag is None else c_diag, ib, vb, nb, k, float(ni.node[k, 1]),
                                         float(ni.node[k, 2]), ni.std[k], SEED, None, FIRST, STRIDE, epi, ni.E, stream_ptr())


def step_inputs(ni, k, epi, special, rs):
    """x_k and model_out (fp32 [N_IMG*epi]) whose x0 is, per image: small with ties (max_val decides), large (the quantile decides), and the
    `special` kind.  x0 = ((-out/std)*sigma^2 + x)/alpha is linear in (x, out): scaling both scales it."""
    x = rs.randn(N_IMG, epi).astype(np.float32)
    out = rs.randn(N_IMG, epi).astype(np.float32)
    x[0], out[0] = x[0] * np.float32(0.05), out[0] * np.float32(0.05)
    x[0, epi // 2:], out[0, epi // 2:] = x[0, :epi - epi // 2], out[0, :epi - epi // 2]          # every value twice: ties
    x[1], out[1] = x[1] * np.float32(4.0), out[1] * np.float32(4.0)
    if special == "zeros":
        x[2], out[2] = 0.0, 0.0
    elif special == "nan":
        out[2, rs.randint(epi)] = np.nan
    elif special == "inf":
        x[2, 0], x[2, epi - 1] = np.inf, -np.inf
    return x.reshape(-1), out.reshape(-1)


@pytest.mark.parametrize("epi", SIZES)
@pytest.mark.parametrize("matrix", ["det5", "sde5"])
def test_fused_step_equals_the_entries_one_after_the_other(dev, matrices, matrix, epi):
    """k = 0 and k = 4 (a full history row in front) of a 5-step matrix: hist[k] == the mirror applied to what natinf_step_f64hist_noise
    wrote on a copy of the slab; x_next == fp32(weighted sum over the corrected slab, diagonal included) + fp32(noise sum), then
    natinf_known_blend_f32 when there are known pixels; x0_s == the mirror's thresholds."""
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    from naturaldiffusion_amd.sampler import CifarNI, known_schedule, x0_threshold_host
    C, B, node = matrices[matrix]
    assert C.shape == (5, 5)
    E = N_IMG * epi
    rs = np.random.RandomState(epi + len(matrix))
    stds = [float(O.vp_std_f32(node[k, 0])) for k in range(5)]
    plain = CifarNI(C, B, node, E, device=dev, stds=stds, seed=SEED, elems_per_image=epi)              # rows, and the slab copy
    assert plain.stochastic == (matrix == "sde5")
    levels = known_schedule(node, "mean")
    zeros = torch.zeros(E, device=dev)
    known = torch.from_numpy(rs.randn(E).astype(np.float32)).to(dev)
    mask = torch.from_numpy((rs.rand(epi) < 0.4).astype(np.uint8) * 255).to(dev)                       # one row shared by every image
    decided_by = set()
    for k, special, (mode, ratio, max_val) in [(0, "zeros", CASES[1]), (0, "nan", CASES[0]), (4, "zeros", CASES[0]), (4, "nan", CASES[1]),
                                               (4, "inf", CASES[1]), (4, "inf", CASES[2]), (4, "zeros", CASES[3]), (4, "zeros", CASES[4])]:
        fix = CifarNI(C, B, node, E, device=dev, stds=stds, seed=SEED, elems_per_image=epi, x0_fix=mode, x0_ratio=ratio, x0_max=max_val)
        h = torch.from_numpy(rs.randn(k, E)).to(dev)
        fix.hist[:k] = h
        plain.hist[:k] = h
        x_np, out_np = step_inputs(plain, k, epi, special, rs)
        x, out = torch.from_numpy(x_np).to(dev), torch.from_numpy(out_np).to(dev)
        noise = torch.from_numpy(rs.randn(E).astype(np.float32)).to(dev)
        # the reference: the unfixed entry on the slab copy, the mirror on its hist[k], then existing entries on the corrected slab
        scratch = torch.empty(E, device=dev)
        assert raw_noise_step(plain, k, x, out, noise, plain.hist, scratch, epi) == 0
        want_h, want_s = x0_threshold_host(plain.hist[k].cpu().numpy().reshape(N_IMG, epi), mode, ratio, max_val)
        plain.hist[k] = torch.from_numpy(want_h.reshape(-1)).to(dev)
        r = plain.rows.rows[k]
        idx = torch.from_numpy(np.append(plain.rows.idx_host[r.start:r.start + r.n], k).astype(np.int32)).to(dev)
        val = torch.from_numpy(np.append(plain.rows.val_host[r.start:r.start + r.n], r.diag).astype(np.float64)).to(dev)
        acc_f = torch.empty(E, device=dev)
        assert lib.natinf_weighted_sum_f64(ptr(plain.hist), ptr(acc_f), ptr(idx), ptr(val), r.n + 1, E, stream_ptr()) == 0
        nacc_f, side = torch.empty(E, device=dev), torch.empty_like(plain.hist)
        assert raw_noise_step(plain, k, zeros, zeros, noise, side, nacc_f, epi, n_terms=0, c_diag=0.0) == 0      # fp32(0) + fp32(noise sum)
        want_x = acc_f + nacc_f                                                                       # one fp32 addition per element
        for with_known in (False, True):
            kw = dict(known=known, mask=mask) if with_known else {}
            got = fix.step(k, x, out, noise, index=(FIRST, STRIDE), **kw)
            ref = want_x
            if with_known:
                a, s, c = levels[k + 1]
                ref = torch.empty_like(want_x)
                assert lib.natinf_known_blend_f32(ptr(want_x), ptr(ref), ptr(known), ptr(mask), epi, 0, a, s, c, SEED, None, FIRST, STRIDE,
                                                  epi, E, stream_ptr()) == 0
            tag = (matrix, epi, k, special, mode, ratio, max_val, with_known)
            assert same_bytes(fix.hist[k], want_h), tag
            assert same_bytes(fix.x0_s[k], want_s), (tag, fix.x0_s[k].cpu().numpy(), want_s)
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), tag                     # torch.equal on the bit patterns: a NaN image compares too
            if special == "zeros":
                assert torch.equal(got, ref) and bool(torch.isfinite(got).all()), tag
            assert same_bytes(fix.hist[:k], h.cpu().numpy()), tag                                     # the rows in front are read, never written
        if mode == "dynamic":
            decided_by |= {"max_val" if v == max_val else "quantile" for v in want_s[:2]}
            if special == "nan":
                assert np.isnan(want_s[2]) and np.isnan(want_h[2]).all()
    assert decided_by == {"max_val", "quantile"}


# ------------------------------------------------------------------------------ 3. a whole trajectory against its mirror on the CPU
@pytest.mark.parametrize("matrix,mode,ratio,max_val", [("det5", "dynamic", 0.995, 1.0), ("sde5", "dynamic", 0.9, 0.5), ("det5", "clip", 0.995, 1.0),
                                                        ("sde5", "clip", 0.995, 0.5)])
def test_run_equals_the_mirror_trajectory(dev, matrices, matrix, mode, ratio, max_val):
    """CifarNI.run over five steps, the model outputs fixed tensors independent of x: every x_k equals, byte for byte, the CPU trajectory built
    from the oracle's pieces with x0_threshold_host between the data prediction and the history."""
    from naturaldiffusion_amd.CIFAR10NaturalInference import philox_noise
    from naturaldiffusion_amd.sampler import CifarNI, x0_threshold_host
    C, B, node = matrices[matrix]
    epi, N = 3072, 5
    E = N_IMG * epi
    gidx = [FIRST + STRIDE * i for i in range(N_IMG)]
    eps = {j: philox_noise(gidx, (epi,), SEED, dev, column=j).cpu().reshape(-1) for j in range(N + 1)}
    stds = [float(O.vp_std_f32(node[k, 0])) for k in range(N)]
    g = torch.Generator().manual_seed(5)
    scale = torch.tensor([0.2, 1.0, 3.0]).repeat_interleave(epi)                                   # per image: under, near and over max_val
    outs = [torch.randn(E, generator=g) * scale for _ in range(N)]
    ni = CifarNI(C, B, node, E, device=dev, stds=stds, seed=SEED, elems_per_image=epi, x0_fix=mode, x0_ratio=ratio, x0_max=max_val)
    calls = []

    def model_fn(x, labels):
        calls.append(1)
        return outs[len(calls) - 1].to(dev).view(x.shape)
    xs = ni.run(model_fn, eps[0].view(N_IMG, 3, 32, 32).to(dev), return_all=True, index=(FIRST, STRIDE))
    assert len(xs) == N + 1 and len(calls) == N
    x, hist, thresholds = eps[0], [], []
    for k in range(N):
        x0 = O.x0_from_score(x, O.score_from_model_out(outs[k], torch.tensor(stds[k])), node[k, 1], node[k, 2])
        assert x0.dtype == torch.float64
        y, s = x0_threshold_host(x0.numpy().reshape(N_IMG, epi), mode, ratio, max_val)
        hist.append(torch.from_numpy(y.reshape(-1)))
        thresholds.append(s)
        m = min(k + 2, B.shape[1]) if ni.stochastic else 1
        x = O.cifar_weighted_sum(C[k], hist) + O.validate_weighted_sum(B[k, :m], [eps[j] for j in range(m)])
        assert x.dtype == torch.float32
        assert same_bytes(xs[k + 1].reshape(-1), x.numpy()), (matrix, mode, k)
        assert same_bytes(ni.hist[k], y), (matrix, mode, k)
    want_s = np.stack(thresholds)
    assert tuple(ni.x0_s.shape) == (N, N_IMG) and same_bytes(ni.x0_s, want_s)
    assert (want_s > max_val).any() if mode == "dynamic" else (want_s == max_val).all()             # (step 0 divides by alpha_0 ~ 0.007: far over max_val)


# ------------------------------------------------------------------------------ 4. refusals
def test_an_image_over_the_cap_is_refused_and_nothing_is_written(dev, matrices):
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr, X0_DYNAMIC
    from naturaldiffusion_amd.sampler import CifarNI
    C, B, node = matrices["det5"]
    epi = 8196
    buf = torch.full((epi,), 3.0, dtype=torch.float64, device=dev)
    assert lib.natinf_x0_threshold_f64(ptr(buf), None, 1, epi, X0_DYNAMIC, 0.995, 1.0, stream_ptr()) == -1
    with pytest.raises(ValueError):
        CifarNI(C, B, node, epi, device=dev, seed=SEED, elems_per_image=epi, x0_fix="dynamic")
    ni = CifarNI(C, B, node, epi, device=dev, seed=SEED, x0_fix="dynamic")                        # elems_per_image left to the step
    t = torch.zeros(epi, device=dev)
    xn = torch.full((epi,), 7.0, device=dev)
    with pytest.raises(ValueError):
        ni.step(0, t, t, t, xn, elems_per_image=epi)
    with pytest.raises(ValueError):
        ni.step(0, t, t, t, xn)                                                                     # no elems_per_image at all
    idx, val, n = ni.rows.ptrs(0)
    ib, vb, nb = ni._noise_rows().ptrs(0)
    args = lambda e, mode: (ptr(t), ptr(t), ptr(t), ptr(ni.hist), ptr(xn), idx, val, n, 1.0, ib, vb, nb, 0, 0.9, 0.4, 0.4, SEED, None, 0, 1, e, epi,
                            None, None, 0, 0, 0.0, 0.0, 0, mode, 0.995, 1.0, None, stream_ptr())
    assert lib.natinf_step_f64hist_x0fix(*args(epi, X0_DYNAMIC)) == -1
    assert lib.natinf_step_f64hist_x0fix(*args(4, 3)) == -1
    torch.cuda.synchronize()
    assert bool((xn == 7.0).all()) and bool((buf == 3.0).all())
    assert lib.natinf_step_f64hist_x0fix(*args(4, X0_DYNAMIC)) == 0                                 # the same call with good arguments goes through
    torch.cuda.synchronize()
    assert not bool((xn == 7.0).any())
    with pytest.raises(ValueError):                                                                 # colorization has no correction
        ni.step(0, t, t, t, xn, elems_per_image=12, gray_u=torch.zeros(epi // 3, device=dev))
