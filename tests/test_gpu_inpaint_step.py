"""GPU tests of the inpainting step of the CIFAR10 form (include/natinf.h: natinf_known_blend_f32, natinf_step_f64hist_inpaint): after the
update of natinf_step_f64hist_noise the known elements are overwritten, in the same launch, with the data diffused to a noise level.  Every
comparison is np.array_equal / byte equality against a numpy restatement fed the library's own natinf_randn_philox_col_f32 columns (as
tests/test_gpu_ni_stochastic.py does for the injected noise), or against the unblended entry followed by the blend entry."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from naturaldiffusion_amd.coeff import load_coeff_npz
from oracle import ni_oracle as O

SEED = 888
COL0 = 2 ** 31
ARRAY_INDEX = [5, 2 ** 32 + 7, 40, 2 ** 33 + 1]                 # one >= 2^32: counter word 1 is in use
FIRST, STRIDE = 11, 3
MATRICES = {"det5": "weights/step_5_weight_00.npz", "sde18": "results/euler_heun/sde_euler_018.npz"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def columns(indices, epi, cols, dev):
    """library columns of the given global indices, flat CPU numpy [n*epi] each"""
    from naturaldiffusion_amd.CIFAR10NaturalInference import philox_noise
    return {j: philox_noise(indices, (epi,), SEED, dev, column=j).cpu().numpy().reshape(-1) for j in cols}


def pattern_mask(n_elem, rs):
    """a mask whose quads run through all 16 byte patterns (quad q: pattern q mod 16), the non-zero bytes taking several values"""
    q = np.arange(n_elem // 4)
    bits = ((q[:, None] % 16) >> np.arange(4)[None, :]) & 1
    vals = rs.choice(np.array([1, 2, 128, 255], dtype=np.uint8), size=bits.shape)
    return (bits.astype(np.uint8) * vals).reshape(-1)


def blend_np(x, known, mask, z, alpha, std):
    """the definition: mask ? fp32(fp32(known*alpha) + fp32(z*std)) : x; std == 0: fp32(known*alpha)"""
    a, s = np.float32(alpha), np.float32(std)
    md = known * a
    assert md.dtype == np.float32
    if s != 0:
        md = md + z * s
    return np.where(mask != 0, md, x)


def tile(row, n_img, stride, epi):
    """the [n_img*epi] array a kernel sees through an image stride: the rows themselves, or the one row repeated"""
    return row if stride else np.tile(row[:epi], n_img)


def raw_blend(x_in, out, known, mask, ks, ms, alpha, std, column, index_args, epi, E, seed=SEED):
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    it, first, stride = index_args
    return lib.natinf_known_blend_f32(ptr(x_in), ptr(out), ptr(known), ptr(mask), ks, ms, alpha, std, column, seed, ptr(it), first, stride,
                                      epi, E, stream_ptr())


def raw_inpaint(ni, k, x, out, noise, xn, index_args, epi, known, mask, ks, ms, alpha, std, column, rows_b=None):
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    idx, val, n = ni.rows.ptrs(k)
    ib, vb, nb = (rows_b or ni._noise_rows()).ptrs(k)
    it, first, stride = index_args
    return lib.natinf_step_f64hist_inpaint(ptr(x), ptr(out), ptr(noise), ptr(ni.hist), ptr(xn), idx, val, n, ni.rows.rows[k].diag, ib, vb, nb,
                                           k, float(ni.node[k, 1]), float(ni.node[k, 2]), ni.std[k], SEED, ptr(it), first, stride, epi, ni.E,
                                           ptr(known), ptr(mask), ks, ms, alpha, std, column, stream_ptr())


def index_forms(form, n_img, dev):
    """(what CifarNI.step takes, (tensor, first, stride) of the C entries, the global indices as a list)"""
    if form == "array":
        idx = ARRAY_INDEX[:n_img]
        t = torch.tensor(idx, dtype=torch.int64, device=dev)
        return t, (t, 0, 0), idx
    return (FIRST, STRIDE), (None, FIRST, STRIDE), [FIRST + STRIDE * i for i in range(n_img)]


# ------------------------------------------------------------------------------ 1. whole trajectories
@pytest.mark.parametrize("per_image", [(True, True), (True, False), (False, True), (False, False)], ids=["kE-mE", "kE-m0", "k0-mE", "k0-m0"])
@pytest.mark.parametrize("form", ["array", "first_stride"])
@pytest.mark.parametrize("n_img,epi", [(4, 3072), (3, 40)])
@pytest.mark.parametrize("matrix", ["det5", "sde18"])
def test_trajectory_fused_equals_step_then_blend_and_the_restatement(dev, repo_root, matrix, n_img, epi, form, per_image):
    """Every step of a trajectory on random model outputs: x_next of the fused entry (through CifarNI.step) == the unblended entry followed by
    natinf_known_blend_f32 == the numpy restatement; hist[k] == the unblended entry's.  The levels are known_schedule's, so the last step is
    the std = 0 form."""
    from naturaldiffusion_amd.sampler import CifarNI, known_schedule
    C, B, node = load_coeff_npz(repo_root / MATRICES[matrix])
    N, E = C.shape[0], n_img * epi
    rs = np.random.RandomState(N + n_img)
    index, index_args, gidx = index_forms(form, n_img, dev)
    eps = columns(gidx, epi, range(N + 1), dev)                                              # the matrix's own columns
    kz = columns(gidx, epi, [COL0 + j for j in range(N + 1)], dev)                           # the known-pixel draws
    levels = known_schedule(node, "mean")
    stds = [float(O.vp_std_f32(node[k, 0])) for k in range(N)]
    kper, mper = per_image
    known_np = rs.randn(E if kper else epi).astype(np.float32)
    mask_np = pattern_mask(E if mper else epi, rs)
    known, mask = torch.from_numpy(known_np).to(dev), torch.from_numpy(mask_np).to(dev)
    ks, ms = (epi if kper else 0), (epi if mper else 0)
    known_full, mask_full = tile(known_np, n_img, kper, epi), tile(mask_np, n_img, mper, epi)
    if mper:
        assert len({tuple(q != 0) for q in mask_np.reshape(-1, 4)}) == min(16, E // 4)
    g = torch.Generator().manual_seed(N)
    outs = [torch.randn(E, generator=g) for _ in range(N)]

    ni = CifarNI(C, B, node, E, device=dev, stds=stds, seed=SEED, elems_per_image=epi)
    ref = CifarNI(C, B, node, E, device=dev, stds=stds, seed=SEED, elems_per_image=epi)
    noise = torch.from_numpy(eps[0]).to(dev)
    x = ni.first_input(noise, known, mask, index=index)
    a0, s0, c0 = levels[0]
    xo = blend_np(eps[0], known_full, mask_full, kz[c0], a0, s0)
    assert np.array_equal(x.cpu().numpy(), xo), "first input"
    hist = []
    for k in range(N):
        out = outs[k].to(dev)
        fused = ni.step(k, x, out, noise, index=index, known=known, mask=mask)
        un = ref.step(k, x, out, noise, index=index) if ref.stochastic else ref.step(k, x, out, noise)     # natinf_step_f64hist_noise / natinf_step_f64hist
        a, s, c = levels[k + 1]
        two = torch.empty_like(un)
        assert raw_blend(un, two, known, mask, ks, ms, a, s, c, index_args, epi, E) == 0
        assert fused.cpu().numpy().tobytes() == two.cpu().numpy().tobytes(), f"step {k}: fused != step + blend"
        assert ni.hist[k].cpu().numpy().tobytes() == ref.hist[k].cpu().numpy().tobytes(), f"step {k}: hist"
        xt = torch.from_numpy(xo)
        hist.append(O.x0_from_score(xt, O.score_from_model_out(outs[k], torch.tensor(stds[k])), node[k, 1], node[k, 2]))
        m = min(k + 2, B.shape[1]) if ref.stochastic else 1
        unblended = O.cifar_weighted_sum(C[k], hist) + O.validate_weighted_sum(B[k, :m], [torch.from_numpy(eps[j]) for j in range(m)])
        assert np.array_equal(un.cpu().numpy(), unblended.numpy()), f"step {k}: unblended restatement"
        xo = blend_np(unblended.numpy(), known_full, mask_full, kz[c], a, s)
        assert np.array_equal(fused.cpu().numpy(), xo), f"step {k}: restatement"
        x = fused
    assert levels[N][1] == 0.0 and np.isfinite(xo).all()


# ------------------------------------------------------------------------------ 2. identities of one step
@pytest.fixture(scope="module")
def one_step(dev, repo_root):
    """step k = 3 of sde_euler_018 with a random history in front of it, 4 images of 3072 elements"""
    from naturaldiffusion_amd.sampler import CifarNI
    C, B, node = load_coeff_npz(repo_root / MATRICES["sde18"])
    n_img, epi, k = 4, 3072, 3
    E = n_img * epi
    g = torch.Generator().manual_seed(2)
    ni = CifarNI(C, B, node, E, device=dev, seed=SEED, elems_per_image=epi)
    ref = CifarNI(C, B, node, E, device=dev, seed=SEED, elems_per_image=epi)
    h = torch.randn(k, E, generator=g, dtype=torch.float64)
    ni.hist[:k] = h.to(dev)
    ref.hist[:k] = h.to(dev)
    t = lambda: torch.randn(E, generator=g).to(dev)
    d = dict(ni=ni, ref=ref, k=k, n_img=n_img, epi=epi, E=E, x=t(), out=t(), noise=t(), known=t())
    d["index_args"] = (torch.tensor(ARRAY_INDEX, dtype=torch.int64, device=dev), 0, 0)
    d["unblended"] = ref.step(k, d["x"], d["out"], d["noise"], index=d["index_args"][0]).clone()
    return d


def test_mask_all_zero_gives_the_bytes_of_the_unblended_entry(dev, one_step):
    s = one_step
    mask = torch.zeros(s["E"], dtype=torch.uint8, device=dev)
    xn = torch.empty(s["E"], device=dev)
    assert raw_inpaint(s["ni"], s["k"], s["x"], s["out"], s["noise"], xn, s["index_args"], s["epi"], s["known"], mask, s["epi"], s["epi"],
                       0.7, 0.3, COL0 + 4) == 0
    assert xn.cpu().numpy().tobytes() == s["unblended"].cpu().numpy().tobytes()
    assert s["ni"].hist[s["k"]].cpu().numpy().tobytes() == s["ref"].hist[s["k"]].cpu().numpy().tobytes()


def test_mask_all_one_with_a_nan_model_output_gives_the_finite_blend(dev, one_step):
    s = one_step
    E, epi, k = s["E"], s["epi"], s["k"]
    mask = torch.full((epi,), 255, dtype=torch.uint8, device=dev)                            # shared row, stride 0
    nan = torch.full((E,), float("nan"), device=dev)
    xn = torch.empty(E, device=dev)
    assert raw_inpaint(s["ni"], k, s["x"], nan, s["noise"], xn, s["index_args"], epi, s["known"], mask, epi, 0, 0.7, 0.3, COL0 + 4) == 0
    z = columns(ARRAY_INDEX, epi, [COL0 + 4], dev)[COL0 + 4]
    want = blend_np(np.full(E, np.nan, np.float32), s["known"].cpu().numpy(), np.ones(E, np.uint8), z, 0.7, 0.3)
    got = xn.cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, want)
    assert torch.isnan(s["ni"].hist[k]).all()                                                # hist[k] is the unblended entry's: NaN
    s["ni"].hist[k] = s["ref"].hist[k]


def test_std_zero_gives_known_times_alpha(dev, one_step):
    s = one_step
    E, epi = s["E"], s["epi"]
    rs = np.random.RandomState(4)
    mask_np = pattern_mask(E, rs)
    mask = torch.from_numpy(mask_np).to(dev)
    xn, alone = torch.empty(E, device=dev), torch.empty(E, device=dev)
    alpha = 0.9993
    assert raw_inpaint(s["ni"], s["k"], s["x"], s["out"], s["noise"], xn, s["index_args"], epi, s["known"], mask, epi, epi, alpha, 0.0, COL0) == 0
    assert raw_blend(s["unblended"], alone, s["known"], mask, epi, epi, alpha, 0.0, COL0, s["index_args"], epi, E) == 0
    want = np.where(mask_np != 0, s["known"].cpu().numpy() * np.float32(alpha), s["unblended"].cpu().numpy())
    assert np.array_equal(xn.cpu().numpy(), want) and np.array_equal(alone.cpu().numpy(), want)
    # alpha 1: the known values themselves, whatever the unknown side holds (known_final="data")
    assert raw_blend(s["unblended"], alone, s["known"], mask, epi, epi, 1.0, 0.0, COL0, s["index_args"], epi, E) == 0
    assert np.array_equal(alone.cpu().numpy(), np.where(mask_np != 0, s["known"].cpu().numpy(), s["unblended"].cpu().numpy()))


def test_blend_in_place_and_more_than_one_block(dev, one_step):
    """x_in == out is allowed; E = 12288 elements is 12 blocks of 256 quads"""
    s = one_step
    E, epi = s["E"], s["epi"]
    mask_np = pattern_mask(E, np.random.RandomState(6))
    mask = torch.from_numpy(mask_np).to(dev)
    buf, out = s["unblended"].clone(), torch.empty(E, device=dev)
    assert raw_blend(s["unblended"], out, s["known"], mask, epi, epi, 0.5, 0.8, COL0 + 9, s["index_args"], epi, E) == 0
    assert raw_blend(buf, buf, s["known"], mask, epi, epi, 0.5, 0.8, COL0 + 9, s["index_args"], epi, E) == 0
    assert buf.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
    z = columns(ARRAY_INDEX, epi, [COL0 + 9], dev)[COL0 + 9]
    assert np.array_equal(out.cpu().numpy(), blend_np(s["unblended"].cpu().numpy(), s["known"].cpu().numpy(), mask_np, z, 0.5, 0.8))


# ------------------------------------------------------------------------------ 3. refusals
def test_refusals_leave_the_output_untouched(dev, one_step):
    from naturaldiffusion_amd._lib import lib, ptr
    s = one_step
    ni, k, E, epi = s["ni"], s["k"], s["E"], s["epi"]
    mask = torch.ones(E + 4, dtype=torch.uint8, device=dev)
    xn = torch.full((E,), 7.0, device=dev)
    idx, val, n = ni.rows.ptrs(k)
    ib, vb, nb = ni.rows_b.ptrs(k)
    good = dict(x=ptr(s["x"]), out=ptr(s["out"]), noise=ptr(s["noise"]), hist=ptr(ni.hist), xn=ptr(xn), idx=idx, val=val, n=n, ib=ib, vb=vb, nb=nb,
                k=k, epi=epi, E=E, known=ptr(s["known"]), mask=ptr(mask), ks=epi, ms=epi, col=COL0)

    def step(**kw):
        a = dict(good, **kw)
        return lib.natinf_step_f64hist_inpaint(a["x"], a["out"], a["noise"], a["hist"], a["xn"], a["idx"], a["val"], a["n"], 0.5, a["ib"], a["vb"], a["nb"],
                                               a["k"], 1.0, 0.5, 1.0, SEED, None, 0, 1, a["epi"], a["E"], a["known"], a["mask"], a["ks"], a["ms"],
                                               0.5, 0.5, a["col"], None)

    def blend(**kw):
        a = dict(good, **kw)
        return lib.natinf_known_blend_f32(a["x"], a["xn"], a["known"], a["mask"], a["ks"], a["ms"], 0.5, 0.5, a["col"], SEED, None, 0, 1,
                                          a["epi"], a["E"], None)

    # what the two entries add
    shared = [dict(known=None), dict(mask=None), dict(ks=4), dict(ks=E), dict(ks=-epi), dict(ms=4), dict(ms=2 * epi), dict(mask=ptr(mask) + 1),
              dict(mask=ptr(mask) + 2), dict(col=COL0 - 1), dict(col=0), dict(col=k + 1)]
    # every refusal of natinf_step_f64hist_noise
    base = [dict(x=None), dict(out=None), dict(noise=None), dict(hist=None), dict(xn=None), dict(idx=None, n=1), dict(val=None, n=1), dict(n=-1),
            dict(ib=None, nb=1), dict(vb=None, nb=1), dict(nb=-1), dict(k=-1), dict(E=E + 2), dict(E=0), dict(epi=6), dict(epi=0), dict(epi=5 * 1024, ks=5 * 1024, ms=5 * 1024),
            dict(epi=4 * 2 ** 32, E=4 * 2 ** 32, ks=4 * 2 ** 32, ms=4 * 2 ** 32)]
    for bad in shared + base:
        assert step(**bad) == -1, bad
    for bad in shared + [dict(x=None), dict(xn=None), dict(E=E + 2), dict(E=0), dict(epi=6), dict(epi=0),
                         dict(epi=4 * 2 ** 32, E=4 * 2 ** 32, ks=4 * 2 ** 32, ms=4 * 2 ** 32)]:
        assert blend(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((xn == 7.0).all())
    assert ni.hist[k].cpu().numpy().tobytes() == s["ref"].hist[k].cpu().numpy().tobytes()       # nothing was launched
    assert step(mask=ptr(mask) + 4, ms=0, ks=0) == 0 and blend() == 0                            # the same calls with good arguments go through
    torch.cuda.synchronize()
    assert not bool((xn == 7.0).all())
    ni.hist[k] = s["ref"].hist[k]


def test_python_refusals(dev, repo_root):
    from naturaldiffusion_amd.sampler import CifarNI
    C, B, node = load_coeff_npz(repo_root / MATRICES["det5"])
    epi, E = 3072, 2 * 3072
    t = torch.zeros(E, device=dev)
    known, mask = torch.zeros(E, device=dev), torch.zeros(E, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        CifarNI(C, B, node, E, device=dev, elems_per_image=epi).step(0, t, t, t, known=known, mask=mask)                # no seed
    with pytest.raises(ValueError):
        CifarNI(C, B, node, E, device=dev, seed=1, fast_f32=True, elems_per_image=epi).step(0, t, t, t, known=known, mask=mask)
    ni = CifarNI(C, B, node, E, device=dev, seed=1)
    with pytest.raises(ValueError):
        ni.step(0, t, t, t, known=known, mask=mask)                                                                       # elems_per_image unknown
    for kw in (dict(known=known), dict(mask=mask), dict(known=known[:8], mask=mask), dict(known=known, mask=mask.cpu()),
               dict(known=known, mask=mask, known_final="sample")):
        with pytest.raises(ValueError):
            ni.step(0, t, t, t, elems_per_image=epi, **kw)
    assert ni.step(0, t, t, t, elems_per_image=epi, known=known, mask=mask) is not None
    torch.cuda.synchronize()
