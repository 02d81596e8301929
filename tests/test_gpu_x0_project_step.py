"""GPU tests of the x0 projection of the CIFAR10 form (include/natinf.h: natinf_x0_project_f64, natinf_step_f64hist_project): the predicted x0
of every image is projected, inside the step's launch, onto the pictures whose s x s block averages are a given low-resolution picture, before
the history and the sum see it.  Every comparison is byte equality: the projection against the numpy mirror (sampler.x0_project_host, itself
pinned to the defined order by tests/test_x0_project_host.py), the fused step against existing entries run one after the other on a copy of the
slab."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from naturaldiffusion_amd import coeffgen as G
from naturaldiffusion_amd.coeff import load_coeff_npz
from oracle import ni_oracle as O

SEED = 888
FIRST, STRIDE = 11, 3
N_IMG = 3
# (C, H, W, s): one quad that straddles two rows of its one block; a width that is no multiple of 4 (quads straddle rows and blocks); one block
# that is a whole plane; not square; the job's own shape at every scale (the small instantiation); 3,456 elements (just over its 3,072); the cap
SHAPES = [(1, 2, 2, 2), (3, 2, 6, 2), (1, 8, 8, 8), (3, 8, 16, 4), (3, 32, 32, 2), (3, 32, 32, 4), (3, 32, 32, 8), (3, 32, 36, 4), (2, 64, 64, 8)]
STEP_SHAPES = [(3, 32, 32, 4), (3, 2, 6, 2), (2, 64, 64, 8)]


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


def same_bytes(t, a):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def kinds(n, nblk, seed):
    """six images and their low-resolution rows: zeros, a mix of +0 and -0, a NaN, one inf, magnitudes of 1e-3 and of 1e3 -> fp64 [6, n], [6, nblk]"""
    rs = np.random.RandomState(seed)
    x, low = rs.randn(6, n), rs.randn(6, nblk)
    x[0], low[0] = 0.0, 0.0
    x[1], low[1] = np.where(rs.rand(n) < 0.5, 0.0, -0.0), np.where(rs.rand(nblk) < 0.5, 0.0, -0.0)
    x[2, rs.randint(n)] = np.nan
    x[3, rs.randint(n)] = np.inf
    x[4], low[4] = x[4] * 1e-3, low[4] * 1e-3
    x[5], low[5] = x[5] * 1e3, low[5] * 1e3
    return x, low


# ------------------------------------------------------------------------------ 1. the projection on its own
@pytest.mark.parametrize("c,h,w,s", SHAPES)
def test_project_entry_equals_the_mirror(dev, c, h, w, s):
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    from naturaldiffusion_amd.sampler import x0_project_host
    n, nblk = c * h * w, c * (h // s) * (w // s)
    x, low = kinds(n, nblk, 7 + n + s)
    for rows, stride in ((low, nblk), (low[5:6], 0), (low[1:2], 0)):            # one row per image; one shared row; a shared row of signed zeros
        want, r = x0_project_host(x, rows, (c, h, w), s)
        # the NaN fills its block; the inf makes d = -inf: its own element inf - inf, the rest of its block -inf
        assert np.isnan(r[2]) and np.isinf(r[3]) and np.isnan(want[2]).sum() == s * s
        assert np.isnan(want[3]).sum() == 1 and np.isinf(want[3]).sum() == s * s - 1
        lo = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
        for with_r in (True, False):
            buf = torch.from_numpy(x.copy()).to(dev)
            r_out = torch.full((6,), -7.0, dtype=torch.float64, device=dev)
            assert lib.natinf_x0_project_f64(ptr(buf), ptr(lo), ptr(r_out) if with_r else None, 6, c, h, w, s, stride, stream_ptr()) == 0
            assert same_bytes(buf, want), (c, h, w, s, stride, with_r)
            assert same_bytes(r_out, r if with_r else np.full(6, -7.0)), (c, h, w, s, stride, r_out.cpu().numpy(), r)
        assert same_bytes(lo, rows)                                              # read, never written


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


def step_inputs(epi, special, rs):
    """x_k and model_out (fp32 [N_IMG*epi]) whose x0 is, per image: small, large, and the `special` kind"""
    x = rs.randn(N_IMG, epi).astype(np.float32)
    out = rs.randn(N_IMG, epi).astype(np.float32)
    x[0], out[0] = x[0] * np.float32(0.05), out[0] * np.float32(0.05)
    x[1], out[1] = x[1] * np.float32(4.0), out[1] * np.float32(4.0)
    if special == "zeros":
        x[2], out[2] = 0.0, 0.0
    elif special == "nan":
        out[2, rs.randint(epi)] = np.nan
    elif special == "inf":
        x[2, rs.randint(epi)] = np.inf
    return x.reshape(-1), out.reshape(-1)


@pytest.mark.parametrize("c,h,w,s", STEP_SHAPES)
@pytest.mark.parametrize("matrix", ["det5", "sde5"])
def test_fused_step_equals_the_entries_one_after_the_other(dev, matrices, matrix, c, h, w, s):
    """k = 0 and k = 4 (a full history row in front) of a 5-step matrix: hist[k] == natinf_step_f64hist_noise followed by natinf_x0_project_f64 on
    a copy of the slab (and == the mirror applied to it); x_next == fp32(weighted sum over the projected slab, diagonal included) + fp32(noise
    sum), composed from existing entries; sr_r == the mirror's."""
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    from naturaldiffusion_amd.sampler import CifarNI, x0_project_host
    C, B, node = matrices[matrix]
    assert C.shape == (5, 5)
    epi, nblk = c * h * w, c * (h // s) * (w // s)
    E = N_IMG * epi
    rs = np.random.RandomState(epi + len(matrix))
    stds = [float(O.vp_std_f32(node[k, 0])) for k in range(5)]
    plain = CifarNI(C, B, node, E, device=dev, stds=stds, seed=SEED, elems_per_image=epi)              # rows, and the slab copy
    sr = CifarNI(C, B, node, E, device=dev, stds=stds, seed=SEED, elems_per_image=epi, sr_scale=s, image_shape=(c, h, w))
    assert plain.stochastic == (matrix == "sde5")
    zeros = torch.zeros(E, device=dev)
    for k, special, shared in [(0, "zeros", False), (0, "nan", True), (4, "zeros", True), (4, "nan", False), (4, "inf", False)]:
        hk = torch.from_numpy(rs.randn(k, E)).to(dev)
        sr.hist[:k] = hk
        plain.hist[:k] = hk
        x_np, out_np = step_inputs(epi, special, rs)
        x, out = torch.from_numpy(x_np).to(dev), torch.from_numpy(out_np).to(dev)
        noise = torch.from_numpy(rs.randn(E).astype(np.float32)).to(dev)
        low_np = rs.randn(1 if shared else N_IMG, nblk) * 2.0
        low = torch.from_numpy(low_np.reshape(-1)).to(dev)
        # the reference: the plain entry on the slab copy, the projection entry on its hist[k], then existing entries on the projected slab
        scratch = torch.empty(E, device=dev)
        assert raw_noise_step(plain, k, x, out, noise, plain.hist, scratch, epi) == 0
        want_h, want_r = x0_project_host(plain.hist[k].cpu().numpy().reshape(N_IMG, epi), low_np, (c, h, w), s)
        r_ref = torch.empty(N_IMG, dtype=torch.float64, device=dev)
        assert lib.natinf_x0_project_f64(ptr(plain.hist[k]), ptr(low), ptr(r_ref), N_IMG, c, h, w, s, 0 if shared else nblk, stream_ptr()) == 0
        assert same_bytes(plain.hist[k], want_h) and same_bytes(r_ref, want_r)
        r = plain.rows.rows[k]
        idx = torch.from_numpy(np.append(plain.rows.idx_host[r.start:r.start + r.n], k).astype(np.int32)).to(dev)
        val = torch.from_numpy(np.append(plain.rows.val_host[r.start:r.start + r.n], r.diag).astype(np.float64)).to(dev)
        acc_f = torch.empty(E, device=dev)
        assert lib.natinf_weighted_sum_f64(ptr(plain.hist), ptr(acc_f), ptr(idx), ptr(val), r.n + 1, E, stream_ptr()) == 0
        nacc_f, side = torch.empty(E, device=dev), torch.empty_like(plain.hist)
        assert raw_noise_step(plain, k, zeros, zeros, noise, side, nacc_f, epi, n_terms=0, c_diag=0.0) == 0      # fp32(0) + fp32(noise sum)
        want_x = acc_f + nacc_f                                                                       # one fp32 addition per element
        got = sr.step(k, x, out, noise, index=(FIRST, STRIDE), low=low)
        tag = (matrix, c, h, w, s, k, special, shared)
        assert same_bytes(sr.hist[k], want_h), tag
        assert same_bytes(sr.sr_r[k], want_r), (tag, sr.sr_r[k].cpu().numpy(), want_r)
        assert torch.equal(got.view(torch.int32), want_x.view(torch.int32)), tag                      # on the bit patterns: a NaN block compares too
        assert same_bytes(sr.hist[:k], hk.cpu().numpy()), tag                                         # the rows in front are read, never written
        if special == "zeros":
            assert bool(torch.isfinite(got).all()), tag
        else:                                                                                         # one block of one image, and no other
            nan, inf = int(np.isnan(want_h[2]).sum()), int(np.isinf(want_h[2]).sum())
            assert (nan, inf) == ((s * s, 0) if special == "nan" else (1, s * s - 1)), tag
            assert np.isnan(want_r[2]) if special == "nan" else np.isposinf(want_r[2]), tag
            assert np.isfinite(want_h[:2]).all() and np.isfinite(want_r[:2]).all(), tag


# ------------------------------------------------------------------------------ 3. a whole trajectory against its mirror on the CPU
@pytest.mark.parametrize("matrix", ["det5", "sde5"])
def test_run_equals_the_mirror_trajectory(dev, matrices, matrix):
    """CifarNI.run over five steps with sr_scale=4, the model outputs fixed tensors independent of x: every x_k equals, byte for byte, the CPU
    trajectory built from the oracle's pieces with x0_project_host between the data prediction and the history; so do sr_r and both results."""
    from naturaldiffusion_amd.CIFAR10NaturalInference import philox_noise
    from naturaldiffusion_amd.sampler import CifarNI, downsample_host, x0_project_host
    C, B, node = matrices[matrix]
    shape, s, epi, N = (3, 32, 32), 4, 3072, 5
    E = N_IMG * epi
    gidx = [FIRST + STRIDE * i for i in range(N_IMG)]
    eps = {j: philox_noise(gidx, (epi,), SEED, dev, column=j).cpu().reshape(-1) for j in range(N + 1)}
    stds = [float(O.vp_std_f32(node[k, 0])) for k in range(N)]
    g = torch.Generator().manual_seed(5)
    scale = torch.tensor([0.2, 1.0, 3.0]).repeat_interleave(epi)
    outs = [torch.randn(E, generator=g) * scale for _ in range(N)]
    low_np = np.random.RandomState(9).uniform(-1, 1, size=(N_IMG, epi // 16))
    low = torch.from_numpy(low_np).to(dev)
    results = {}
    for sr_final in ("step", "x0"):
        ni = CifarNI(C, B, node, E, device=dev, stds=stds, seed=SEED, elems_per_image=epi, sr_scale=s, image_shape=shape)
        calls = []

        def model_fn(x, labels):
            calls.append(1)
            return outs[len(calls) - 1].to(dev).view(x.shape)
        xs = ni.run(model_fn, eps[0].view(N_IMG, 3, 32, 32).to(dev), return_all=True, index=(FIRST, STRIDE), low=low.view(N_IMG, 3, 8, 8),
                    sr_final=sr_final)
        assert len(xs) == N + 1 + (sr_final == "x0") and len(calls) == N
        results[sr_final] = xs
    assert all(torch.equal(a, b) for a, b in zip(results["step"], results["x0"]))
    xs = results["x0"]
    x, hist, rs_ = eps[0], [], []
    for k in range(N):
        x0 = O.x0_from_score(x, O.score_from_model_out(outs[k], torch.tensor(stds[k])), node[k, 1], node[k, 2])
        assert x0.dtype == torch.float64
        y, r = x0_project_host(x0.numpy().reshape(N_IMG, epi), low_np, shape, s)
        hist.append(torch.from_numpy(y.reshape(-1)))
        rs_.append(r)
        m = min(k + 2, B.shape[1]) if ni.stochastic else 1
        x = O.cifar_weighted_sum(C[k], hist) + O.validate_weighted_sum(B[k, :m], [eps[j] for j in range(m)])
        assert x.dtype == torch.float32
        assert same_bytes(xs[k + 1].reshape(-1), x.numpy()), (matrix, k)
        assert same_bytes(ni.hist[k], y), (matrix, k)
    assert tuple(ni.sr_r.shape) == (N, N_IMG) and same_bytes(ni.sr_r, np.stack(rs_))
    assert (np.stack(rs_) > 0).all()
    last = hist[-1].to(torch.float32)
    assert same_bytes(xs[N + 1].reshape(-1), last.numpy())
    # the "x0" result has the block means of the data: |A fp32(y) - low| <= 2^-23 M, M = max(|y|, |low|) of the image
    y32 = last.numpy().astype(np.float64).reshape(N_IMG, epi)
    M = np.maximum(np.abs(y32).max(1), np.abs(low_np).max(1))[:, None]
    assert (np.abs(downsample_host(y32, shape, s) - low_np) <= 2.0 ** -23 * M).all()
    # while x_N need not
    xN = xs[N].cpu().numpy().astype(np.float64).reshape(N_IMG, epi)
    assert (np.abs(downsample_host(xN, shape, s) - low_np) > 2.0 ** -23 * M).any()


# ------------------------------------------------------------------------------ 4. refusals
def test_refusals_through_the_abi_and_the_good_call_after_each(dev, matrices):
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    from naturaldiffusion_amd.sampler import CifarNI
    C, B, node = matrices["det5"]
    c, h, w, s = 3, 2, 6, 2
    epi, nblk = 36, 9
    ni = CifarNI(C, B, node, epi, device=dev, seed=SEED, elems_per_image=epi, sr_scale=s, image_shape=(c, h, w))
    t = torch.zeros(epi, device=dev)
    low = torch.ones(nblk, dtype=torch.float64, device=dev)
    xn = torch.full((epi,), 7.0, device=dev)
    buf = torch.full((epi,), 3.0, dtype=torch.float64, device=dev)
    idx, val, n = ni.rows.ptrs(0)
    ib, vb, nb = ni._noise_rows().ptrs(0)

    def step(**kw):
        a = dict(low=ptr(low), ls=nblk, c=c, h=h, w=w, s=s, epi=epi, E=epi)
        a.update(kw)
        return lib.natinf_step_f64hist_project(ptr(t), ptr(t), ptr(t), ptr(ni.hist), ptr(xn), idx, val, n, 1.0, ib, vb, nb, 0, 0.9, 0.4, 0.4, SEED,
                                               None, 0, 1, a["epi"], a["E"], a["low"], a["ls"], a["c"], a["h"], a["w"], a["s"], None, stream_ptr())

    def project(**kw):
        a = dict(low=ptr(low), ls=nblk, c=c, h=h, w=w, s=s)
        a.update(kw)
        return lib.natinf_x0_project_f64(ptr(buf), a["low"], None, 1, a["c"], a["h"], a["w"], a["s"], a["ls"], stream_ptr())
    for bad in (dict(low=None), dict(s=3), dict(s=4), dict(c=0), dict(h=3), dict(w=5), dict(ls=8), dict(c=1), dict(c=300, h=64, w=64)):
        assert step(**bad) == -1, bad
        if bad != dict(c=1):                                                     # (a smaller image is a good call for the entry without elems_per_image)
            assert project(**bad) == -1, bad
        torch.cuda.synchronize()
        assert bool((xn == 7.0).all()) and bool((buf == 3.0).all()), bad
        assert step() == 0 and project() == 0                                    # the same calls with good arguments go through
        torch.cuda.synchronize()
        assert not bool((xn == 7.0).any()) and bool((buf == 1.0).all()), bad     # x0 = 0 projected onto low = 1; buf: 3 + (1 - 3)
        xn.fill_(7.0)
        buf.fill_(3.0)
    # the sampler refuses what it does not compose with, and a low of the wrong size or type
    for kw in (dict(known=t, mask=t.to(torch.uint8)), dict(gray_u=torch.zeros(epi // 3, device=dev))):
        with pytest.raises(ValueError):
            ni.step(0, t, t, t, xn, low=low, **kw)
    for bad_low in (None, low.float(), low[:8], torch.ones(nblk, dtype=torch.float64), low.view(3, 3)):
        with pytest.raises(ValueError):
            ni.step(0, t, t, t, xn, low=bad_low)
    with pytest.raises(ValueError):
        CifarNI(C, B, node, epi, device=dev, seed=SEED, elems_per_image=epi).step(0, t, t, t, xn, low=low)
    assert bool((xn == 7.0).all())
