"""GPU tests of the colorization step of the CIFAR10 form (include/natinf.h: natinf_color_blend_f32, natinf_step_f64hist_colorize): after the
update of natinf_step_f64hist_noise the gray channel of a rotated colour space is overwritten, in the same launch, with the gray data diffused to
a noise level.  Every comparison is np.array_equal / byte equality: the blend against sampler.color_blend_host fed the library's own
natinf_randn_philox_col_f32 plane-0 column, the fused step against the unblended entry followed by the blend entry.

Shapes (elems_per_image, images): (12, 5) one pixel quad per image, five threads; (780, 3) a plane stride of 65 quads, no power of two, and a
partial block; (3072, 3) CIFAR10, three blocks."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from naturaldiffusion_amd.coeff import load_coeff_npz
from oracle import ni_oracle as O

SEED = 888
COL0 = 2 ** 31 + 2 ** 30
FIRST, STRIDE = 2 ** 32 + 7, 3                                  # >= 2^32: counter word 1 is in use
SHAPES = [(12, 5), (780, 3), (3072, 3)]
MATRICES = {"det5": "weights/step_5_weight_00.npz", "sde18": "results/euler_heun/sde_euler_018.npz"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def f9(m):
    return (ctypes.c_float * 9)(*np.asarray(m, np.float32).reshape(-1).tolist())


def matrices():
    from naturaldiffusion_amd.sampler import COLOR_M, COLOR_W
    return f9(COLOR_M), f9(COLOR_W)


def indices(n_img):
    return [FIRST + STRIDE * i for i in range(n_img)]


def plane0(n_img, epi, cols, dev):
    """the library's column of plane 0 of the images FIRST + i*STRIDE, CPU numpy [n_img, P] per column"""
    from naturaldiffusion_amd.CIFAR10NaturalInference import philox_noise
    return {c: philox_noise(indices(n_img), (epi,), SEED, dev, column=c).cpu().numpy()[:, :epi // 3].copy() for c in cols}


def host_blend(x, gray, n_img, epi, alpha, std, z0):
    """color_blend_host on a flat [n_img*epi] array; `gray` flat, n_img rows or one"""
    from naturaldiffusion_amd.sampler import color_blend_host
    P = epi // 3
    return color_blend_host(x.reshape(n_img, 3, P), gray.reshape(-1, P), alpha, std, z0).reshape(-1)


def raw_blend(x_in, out, gray, gs, alpha, std, column, index_args, epi, E, basis=None, inverse=None):
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    M, W = matrices()
    it, first, stride = index_args
    return lib.natinf_color_blend_f32(ptr(x_in), ptr(out), ptr(gray), gs, basis or M, inverse or W, alpha, std, column, SEED, ptr(it), first,
                                      stride, epi, E, stream_ptr())


def step_head(ni, k, x, out, noise, xn, index_args, epi):
    from naturaldiffusion_amd._lib import ptr
    idx, val, n = ni.rows.ptrs(k)
    ib, vb, nb = ni._noise_rows().ptrs(k)
    it, first, stride = index_args
    return (ptr(x), ptr(out), ptr(noise), ptr(ni.hist), ptr(xn), idx, val, n, ni.rows.rows[k].diag, ib, vb, nb, k, float(ni.node[k, 1]),
            float(ni.node[k, 2]), ni.std[k], SEED, ptr(it), first, stride, epi, ni.E)


def raw_noise_step(ni, k, x, out, noise, xn, index_args, epi):
    from naturaldiffusion_amd._lib import lib, stream_ptr
    return lib.natinf_step_f64hist_noise(*step_head(ni, k, x, out, noise, xn, index_args, epi), stream_ptr())


def raw_colorize(ni, k, x, out, noise, xn, index_args, epi, gray, gs, alpha, std, column):
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    M, W = matrices()
    return lib.natinf_step_f64hist_colorize(*step_head(ni, k, x, out, noise, xn, index_args, epi), ptr(gray), gs, M, W, alpha, std, column,
                                            stream_ptr())


# ------------------------------------------------------------------------------ 1. the blend alone
@pytest.mark.parametrize("epi,n_img", SHAPES)
def test_blend_equals_the_host_replay_bit_for_bit(dev, epi, n_img):
    E, P = n_img * epi, epi // 3
    rs = np.random.RandomState(epi)
    x_np, gray_np = rs.randn(E).astype(np.float32), rs.randn(n_img * P).astype(np.float32)
    x, gray = torch.from_numpy(x_np).to(dev), torch.from_numpy(gray_np).to(dev)
    col = COL0 + 9
    z = plane0(n_img, epi, [col], dev)[col]
    ia = (None, FIRST, STRIDE)
    out = torch.full((E,), 7.0, device=dev)
    assert raw_blend(x, out, gray, P, 0.5, 0.8, col, ia, epi, E) == 0
    want = host_blend(x_np, gray_np, n_img, epi, 0.5, 0.8, z)
    assert np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(x.cpu(), torch.from_numpy(x_np))                                      # the input is left alone
    buf = x.clone()                                                                          # in place
    assert raw_blend(buf, buf, gray, P, 0.5, 0.8, col, ia, epi, E) == 0
    assert buf.cpu().numpy().tobytes() == want.tobytes()
    it = torch.tensor(indices(n_img), dtype=torch.int64, device=dev)                         # the global indices as an array
    arr = torch.empty(E, device=dev)
    assert raw_blend(x, arr, gray, P, 0.5, 0.8, col, (it, 0, 0), epi, E) == 0
    assert arr.cpu().numpy().tobytes() == want.tobytes()
    one, rep = torch.empty(E, device=dev), torch.empty(E, device=dev)                        # stride 0 == the one row repeated
    tiled = np.tile(gray_np[:P], n_img)
    assert raw_blend(x, one, gray[:P].contiguous(), 0, 0.5, 0.8, col, ia, epi, E) == 0
    assert raw_blend(x, rep, torch.from_numpy(tiled).to(dev), P, 0.5, 0.8, col, ia, epi, E) == 0
    assert one.cpu().numpy().tobytes() == rep.cpu().numpy().tobytes()
    assert np.array_equal(one.cpu().numpy(), host_blend(x_np, gray_np[:P], n_img, epi, 0.5, 0.8, z))
    nod = torch.empty(E, device=dev)                                                         # std 0: no draw, fp32(gray_u*alpha) rotated back
    assert raw_blend(x, nod, gray, P, 0.9993, 0.0, col, ia, epi, E) == 0
    got = nod.cpu().numpy()
    assert np.array_equal(got, host_blend(x_np, gray_np, n_img, epi, 0.9993, 0.0, None)) and not np.array_equal(got, want)
    assert raw_blend(x, out, gray, P, 0.9993, 0.0, col + 1, ia, epi, E) == 0                 # ... whatever the column
    assert out.cpu().numpy().tobytes() == got.tobytes()


def test_a_nan_reaches_the_three_outputs_of_its_pixel_only(dev):
    epi, n_img = 780, 3
    E, P = n_img * epi, epi // 3
    rs = np.random.RandomState(1)
    x_np, gray_np = rs.randn(E).astype(np.float32), rs.randn(n_img * P).astype(np.float32)
    x_np[epi + P + 77] = np.nan                                                              # image 1, plane 1, pixel 77
    out = torch.empty(E, device=dev)
    assert raw_blend(torch.from_numpy(x_np).to(dev), out, torch.from_numpy(gray_np).to(dev), P, 0.5, 0.0, COL0, (None, 0, 1), epi, E) == 0
    bad = np.flatnonzero(np.isnan(out.cpu().numpy()))
    assert bad.tolist() == [epi + 77, epi + P + 77, epi + 2 * P + 77]


# ------------------------------------------------------------------------------ 2. whole trajectories of the fused step
@pytest.mark.parametrize("shared", [False, True], ids=["gE", "g0"])
@pytest.mark.parametrize("epi,n_img", SHAPES)
@pytest.mark.parametrize("matrix", ["det5", "sde18"])
def test_trajectory_fused_equals_noise_step_then_blend(dev, repo_root, matrix, epi, n_img, shared):
    """Every step of a trajectory on random model outputs: x_next of the fused entry (through CifarNI.step) == natinf_step_f64hist_noise followed by
    natinf_color_blend_f32 == the host replay of the blend on the unblended x_next; hist[k] == the noise step's; a global-index array gives the
    bytes of first_index / index_stride.  The levels are color_schedule's, so the last step is the std = 0 form."""
    from naturaldiffusion_amd.sampler import CifarNI, color_schedule
    C, B, node = load_coeff_npz(repo_root / MATRICES[matrix])
    N, E, P = C.shape[0], n_img * epi, epi // 3
    rs = np.random.RandomState(N + n_img)
    levels = color_schedule(node, "mean")
    kz = plane0(n_img, epi, [lv[2] for lv in levels], dev)
    stds = [float(O.vp_std_f32(node[k, 0])) for k in range(N)]
    gray_np = rs.randn(P if shared else n_img * P).astype(np.float32)
    gray = torch.from_numpy(gray_np).to(dev)
    gs = 0 if shared else P
    noise_np = rs.randn(E).astype(np.float32)
    noise = torch.from_numpy(noise_np).to(dev)
    g = torch.Generator().manual_seed(N)
    outs = [torch.randn(E, generator=g).to(dev) for _ in range(N)]
    ia = (None, FIRST, STRIDE)
    it = torch.tensor(indices(n_img), dtype=torch.int64, device=dev)

    ni, ref, arr = (CifarNI(C, B, node, E, device=dev, stds=stds, seed=SEED, elems_per_image=epi) for _ in range(3))
    x = ni.first_input(noise, index=(FIRST, STRIDE), gray_u=gray)
    a0, s0, c0 = levels[0]
    assert c0 == COL0 and np.array_equal(x.cpu().numpy(), host_blend(noise_np, gray_np, n_img, epi, a0, s0, kz[c0])), "first input"
    for k in range(N):
        a, s, c = levels[k + 1]
        fused = ni.step(k, x, outs[k], noise, index=(FIRST, STRIDE), gray_u=gray)
        un, two, by_array = torch.empty(E, device=dev), torch.empty(E, device=dev), torch.empty(E, device=dev)
        assert raw_noise_step(ref, k, x, outs[k], noise, un, ia, epi) == 0
        assert raw_blend(un, two, gray, gs, a, s, c, ia, epi, E) == 0
        assert fused.cpu().numpy().tobytes() == two.cpu().numpy().tobytes(), f"step {k}: fused != step + blend"
        assert ni.hist[k].cpu().numpy().tobytes() == ref.hist[k].cpu().numpy().tobytes(), f"step {k}: hist"
        assert np.array_equal(fused.cpu().numpy(), host_blend(un.cpu().numpy(), gray_np, n_img, epi, a, s, kz[c])), f"step {k}: host replay"
        assert raw_colorize(arr, k, x, outs[k], noise, by_array, (it, 0, 0), epi, gray, gs, a, s, c) == 0
        assert by_array.cpu().numpy().tobytes() == fused.cpu().numpy().tobytes(), f"step {k}: index array"
        assert arr.hist[k].cpu().numpy().tobytes() == ref.hist[k].cpu().numpy().tobytes(), f"step {k}: hist, index array"
        x = fused.clone()
    assert levels[N][1] == 0.0 and bool(torch.isfinite(x).all())


# ------------------------------------------------------------------------------ 3. refusals
def test_refusals_leave_the_output_untouched(dev, repo_root):
    from naturaldiffusion_amd._lib import lib, ptr
    from naturaldiffusion_amd.sampler import CifarNI
    C, B, node = load_coeff_npz(repo_root / MATRICES["sde18"])
    n_img, epi, k = 3, 3072, 3
    E, P = n_img * epi, epi // 3
    g = torch.Generator().manual_seed(2)
    ni = CifarNI(C, B, node, E, device=dev, seed=SEED, elems_per_image=epi)
    ni.hist[:k + 1] = torch.randn(k + 1, E, generator=g, dtype=torch.float64).to(dev)
    before = ni.hist[k].cpu().numpy().tobytes()
    t = lambda n=E: torch.randn(n, generator=g).to(dev)
    x, out, noise, gray = t(), t(), t(), t(n_img * P)
    xn = torch.full((E,), 7.0, device=dev)                                                   # the poisoned output
    M, W = matrices()
    idx, val, n = ni.rows.ptrs(k)
    ib, vb, nb = ni.rows_b.ptrs(k)
    good = dict(x=ptr(x), out=ptr(out), noise=ptr(noise), hist=ptr(ni.hist), xn=ptr(xn), idx=idx, val=val, n=n, ib=ib, vb=vb, nb=nb,
                k=k, epi=epi, E=E, gray=ptr(gray), gs=P, M=M, W=W, col=COL0)

    def step(**kw):
        a = dict(good, **kw)
        return lib.natinf_step_f64hist_colorize(a["x"], a["out"], a["noise"], a["hist"], a["xn"], a["idx"], a["val"], a["n"], 0.5, a["ib"], a["vb"],
                                                a["nb"], a["k"], 1.0, 0.5, 1.0, SEED, None, 0, 1, a["epi"], a["E"], a["gray"], a["gs"], a["M"],
                                                a["W"], 0.5, 0.5, a["col"], None)

    def blend(**kw):
        a = dict(good, **kw)
        return lib.natinf_color_blend_f32(a["x"], a["xn"], a["gray"], a["gs"], a["M"], a["W"], 0.5, 0.5, a["col"], SEED, None, 0, 1,
                                          a["epi"], a["E"], None)

    # what the two entries add: a NULL gray_u / basis / inverse, an image that is not three planes of whole quads (1024 = 4 mod 12, and divides E),
    # a stride that is neither 0 nor elems_per_image / 3, a column below the colorization family (a matrix's, an inpainting draw's)
    shared = [dict(gray=None), dict(M=None), dict(W=None), dict(epi=1024, gs=0), dict(epi=16, gs=0), dict(gs=4), dict(gs=epi), dict(gs=-P),
              dict(gs=2 * P), dict(col=COL0 - 1), dict(col=2 ** 31), dict(col=2 ** 31 + k + 1), dict(col=0), dict(col=k + 1)]
    # every refusal of natinf_step_f64hist_noise
    base = [dict(x=None), dict(out=None), dict(noise=None), dict(hist=None), dict(xn=None), dict(idx=None, n=1), dict(val=None, n=1), dict(n=-1),
            dict(ib=None, nb=1), dict(vb=None, nb=1), dict(nb=-1), dict(k=-1), dict(E=E + 2), dict(E=0), dict(epi=6, gs=0), dict(epi=0, gs=0),
            dict(epi=5 * 1536, gs=0), dict(epi=12 * 2 ** 32, E=12 * 2 ** 32, gs=0)]
    for bad in shared + base:
        assert step(**bad) == -1, bad
    for bad in shared + [dict(x=None), dict(xn=None), dict(E=E + 2), dict(E=0), dict(epi=6, gs=0), dict(epi=0, gs=0), dict(epi=5 * 1536, gs=0),
                         dict(epi=12 * 2 ** 32, E=12 * 2 ** 32, gs=0)]:
        assert blend(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((xn == 7.0).all())
    assert ni.hist[k].cpu().numpy().tobytes() == before                                      # nothing was launched
    assert step() == 0                                                                       # the same calls with good arguments go through
    torch.cuda.synchronize()
    assert not bool((xn == 7.0).any())
    xn.fill_(7.0)
    assert blend(gs=0, col=2 ** 32 - 1) == 0
    torch.cuda.synchronize()
    assert not bool((xn == 7.0).any())


def test_python_refusals(dev, repo_root):
    from naturaldiffusion_amd.sampler import CifarNI
    C, B, node = load_coeff_npz(repo_root / MATRICES["det5"])
    epi, E = 3072, 2 * 3072
    t = torch.zeros(E, device=dev)
    gray = torch.zeros(E // 3, device=dev)
    known, mask = torch.zeros(E, device=dev), torch.zeros(E, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        CifarNI(C, B, node, E, device=dev, elems_per_image=epi).step(0, t, t, t, gray_u=gray)                             # no seed
    with pytest.raises(ValueError):
        CifarNI(C, B, node, E, device=dev, seed=1, fast_f32=True, elems_per_image=epi).step(0, t, t, t, gray_u=gray)
    ni = CifarNI(C, B, node, E, device=dev, seed=1)
    with pytest.raises(ValueError):
        ni.step(0, t, t, t, gray_u=gray)                                                                                  # elems_per_image unknown
    for kw in (dict(gray_u=gray[:8]), dict(gray_u=gray.cpu()), dict(gray_u=gray, known=known, mask=mask), dict(gray_u=gray, mask=mask),
               dict(gray_u=gray, known_final="sample"), dict(gray_u=gray.double())):
        with pytest.raises(ValueError):
            ni.step(0, t, t, t, elems_per_image=epi, **kw)
    for kw in (dict(gray_u=gray, known=known, mask=mask), dict(gray_u=gray[:8])):
        with pytest.raises(ValueError):
            ni.first_input(t, elems_per_image=epi, **kw)
    with pytest.raises(ValueError):
        ni.run(lambda x, lab: x, t.view(2, 3, 32, 32), gray_u=gray, known=known, mask=mask)
    assert ni.step(0, t, t, t, elems_per_image=epi, gray_u=gray) is not None
    torch.cuda.synchronize()
