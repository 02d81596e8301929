"""Host pieces of the x0 correction of the CIFAR10 form (no GPU): the numpy mirror of the arithmetic contract against the reference's own
``dynamic_thresholding_fn`` (a recorded fixture) and against torch evaluated live, the refusals of the two ABI entries, which touch no device,
and the refusals of the sampler and the job, which all come before any GPU call."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from naturaldiffusion_amd import _lib
from naturaldiffusion_amd.CIFAR10NaturalInference import BatchLanes, generate_sharded, natural_inference_tx, prepare_gray, prepare_known
from naturaldiffusion_amd.sampler import CifarNI, check_x0_fix, x0_threshold_host

lib = _lib.lib
EPI = 3 * 32 * 32
EINVAL = -1


def _bits(a):
    """the uint64 view with every NaN counted equal to every NaN"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


# ------------------------------------------------------------------------------ 1. the mirror against the reference's recorded outputs
@pytest.fixture(scope="module")
def golden(repo_root):
    return np.load(repo_root / "tests/golden/x0_threshold.npz")


@pytest.mark.parametrize("n", [3072, 4, 8, 260])
def test_mirror_reproduces_the_reference_fixture(golden, n):
    x, cases, ys = golden[f"x_{n}"], golden[f"cases_{n}"], golden[f"y_{n}"]
    assert x.dtype == np.float64 and x.shape == (6, n) and ys.shape == (len(cases), 6, n)
    assert {tuple(c) for c in cases} >= {(0.995, 1.0), (0.5, 1.0), (0.0, 1.0), (1.0, 1.0), (0.995, 0.5), (0.5, 0.5)}
    assert np.isnan(x[2]).sum() == 1 and np.isinf(x[3]).sum() == 2 and not x[1].any() and len(np.unique(x[0])) <= 13
    decided_by = set()
    for (ratio, max_val), want in zip(cases, ys):
        got, s = x0_threshold_host(x, "dynamic", ratio, max_val)
        assert got.dtype == np.float64 and np.array_equal(_bits(got), _bits(want)), (n, ratio, max_val)
        assert np.isnan(s[2]) and s[1] == max_val
        decided_by |= {"max_val" if v == max_val else "quantile" for v in s[[0, 4, 5]]}
    assert decided_by == {"max_val", "quantile"}


# ------------------------------------------------------------------------------ 2. the mirror against torch's three statements, live
@pytest.mark.parametrize("n,ratio", [(3072, 0.995), (3072, 0.5), (260, 0.995), (260, 0.3), (8, 0.995), (4, 0.7), (1000, 0.999), (8192, 0.995)])
def test_mirror_equals_torch_bit_for_bit(n, ratio):
    rs = np.random.RandomState(n + int(ratio * 1000))
    x = rs.randn(24, n) * np.geomspace(0.01, 8.0, 24)[:, None]               # some rows under max_val, some over
    x[3, ::2] = x[3, 1::2]                                                   # ties
    for max_val in (1.0, 0.5):
        xt = torch.from_numpy(x.copy())
        s = torch.quantile(torch.abs(xt), ratio, dim=1)
        s = torch.maximum(s, max_val * torch.ones_like(s))[:, None]
        want = torch.clamp(xt, -s, s) / s
        got, gs = x0_threshold_host(x, "dynamic", ratio, max_val)
        assert np.array_equal(gs.view(np.uint64), s[:, 0].numpy().view(np.uint64))
        assert np.array_equal(got.view(np.uint64), want.numpy().view(np.uint64))
        assert (gs == max_val).any() and (gs > max_val).any()


def test_clip_mirror():
    x = np.array([[-3.0, -1.0, -0.0, 0.25], [1.0, 1.5, np.inf, -np.inf]])
    x[0, 3] = np.float64(np.nan)
    y, s = x0_threshold_host(x, "clip", 0.995, 1.0)
    assert np.array_equal(_bits(y), _bits(np.array([[-1.0, -1.0, -0.0, np.nan], [1.0, 1.0, 1.0, -1.0]]))) and s.tolist() == [1.0, 1.0]
    want = torch.clamp(torch.from_numpy(x), -0.5, 0.5).numpy()
    assert np.array_equal(_bits(x0_threshold_host(x, 1, 0.0, 0.5)[0]), _bits(want))
    one, s1 = x0_threshold_host(x[1], "dynamic", 1.0, 1.0)                   # one image as a vector; inf - inf inside the quantile
    assert one.shape == (4,) and np.isnan(s1).all() and np.isnan(one).all()
    for bad in (dict(mode="static"), dict(mode=3), dict(ratio=1.5), dict(ratio=float("nan")), dict(max_val=0.0), dict(max_val=float("inf"))):
        a = dict(mode="dynamic", ratio=0.5, max_val=1.0)
        a.update(bad)
        with pytest.raises(ValueError):
            x0_threshold_host(x, a["mode"], a["ratio"], a["max_val"])


# ------------------------------------------------------------------------------ 3. the ABI: exported, signed, and every refusal without a device
def test_library_exports_and_signs_both_entries():
    for name, n_args in (("natinf_x0_threshold_f64", 8), ("natinf_step_f64hist_x0fix", 34)):
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        assert res is C.c_int and len(args) == n_args and fn.restype is C.c_int and list(fn.argtypes) == list(args)
    inpaint = _lib.SIGNATURES["natinf_step_f64hist_inpaint"][1]
    fix = _lib.SIGNATURES["natinf_step_f64hist_x0fix"][1]
    assert list(fix) == list(inpaint[:-1]) + [C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]      # inpaint's list, stream last
    assert (_lib.X0_CLIP, _lib.X0_DYNAMIC) == (1, 2)


P = 4096                                                                     # a dummy non-NULL, 16-byte aligned address: no refused call reads it


def _threshold(**kw):
    a = dict(x0=P, s_out=P, n_images=3, epi=EPI, mode=2, ratio=0.995, max_val=1.0)
    a.update(kw)
    return lib.natinf_x0_threshold_f64(a["x0"], a["s_out"], a["n_images"], a["epi"], a["mode"], a["ratio"], a["max_val"], None)


def _step(**kw):
    a = dict(x_k=P, model_out=P, noise=P, hist=P, x_next=P, idx=P, val=P, n_terms=2, c_diag=1.0, idx_b=P, val_b=P, n_b=1, k=2, alpha=0.9,
             sigma=0.4, std=0.4, seed=7, index=None, first=0, stride=1, epi=EPI, E=3 * EPI, known=None, mask=None, ks=0, ms=0, ka=0.0, kstd=0.0,
             kcol=0, mode=2, ratio=0.995, max_val=1.0, s_out=None)
    a.update(kw)
    return lib.natinf_step_f64hist_x0fix(a["x_k"], a["model_out"], a["noise"], a["hist"], a["x_next"], a["idx"], a["val"], a["n_terms"],
                                         a["c_diag"], a["idx_b"], a["val_b"], a["n_b"], a["k"], a["alpha"], a["sigma"], a["std"], a["seed"],
                                         a["index"], a["first"], a["stride"], a["epi"], a["E"], a["known"], a["mask"], a["ks"], a["ms"],
                                         a["ka"], a["kstd"], a["kcol"], a["mode"], a["ratio"], a["max_val"], a["s_out"], None)


BAD_FIX = [dict(mode=0), dict(mode=3), dict(mode=-1), dict(ratio=-0.001), dict(ratio=1.001), dict(ratio=float("nan")), dict(max_val=0.0),
           dict(max_val=-1.0), dict(max_val=float("inf")), dict(max_val=float("nan"))]


def test_threshold_entry_refusals_touch_no_device():
    for bad in BAD_FIX + [dict(x0=None), dict(n_images=0), dict(n_images=-2), dict(epi=0), dict(epi=6), dict(epi=-4), dict(epi=8196),
                          dict(epi=2 ** 20)]:
        assert _threshold(**bad) == EINVAL, bad
    assert _threshold(mode=1, ratio=2.0) == EINVAL                           # the ratio is checked in CLIP mode too


def test_step_entry_refusals_touch_no_device():
    for bad in BAD_FIX:
        assert _step(**bad) == EINVAL, bad
    # every refusal of natinf_step_f64hist_inpaint that does not concern the blend
    for bad in (dict(x_k=None), dict(model_out=None), dict(noise=None), dict(hist=None), dict(x_next=None), dict(idx=None), dict(val=None),
                dict(n_terms=-1), dict(idx_b=None), dict(val_b=None), dict(n_b=-1), dict(k=-1), dict(E=0), dict(E=3 * EPI + 2), dict(epi=0),
                dict(epi=6, E=24), dict(epi=EPI, E=EPI + 4), dict(epi=8196, E=8196), dict(epi=16384, E=16384)):
        assert _step(**bad) == EINVAL, bad
    # exactly one of known / mask
    assert _step(known=P) == EINVAL and _step(mask=P) == EINVAL
    # with both given, the blend's refusals apply ...
    ok = dict(known=P, mask=P, ks=EPI, ms=0, ka=0.5, kstd=0.5, kcol=2 ** 31 + 3)
    for bad in (dict(ks=8), dict(ms=EPI + 4), dict(mask=P + 2), dict(kcol=5), dict(kcol=2 ** 31 - 1)):
        assert _step(**dict(ok, **bad)) == EINVAL, bad
    assert _step(**dict(ok, mode=7)) == EINVAL
    # ... and with both NULL they do not: nothing but the bad mode refuses this call (strides and column the blend would refuse)
    assert _step(ks=8, ms=12, kcol=5, mode=0) == EINVAL


# ------------------------------------------------------------------------------ 4. the sampler and the job refuse on the host
def test_check_x0_fix():
    assert check_x0_fix(None, "x", -1) == 0                                  # no correction: nothing else is looked at
    assert check_x0_fix("clip", 0.995, 1.0) == 1 and check_x0_fix("dynamic", 0, 0.5) == 2 and check_x0_fix("dynamic", 1, 2, elems_per_image=8192) == 2
    for bad in (dict(x0_fix="static"), dict(x0_fix=2), dict(x0_fix=True), dict(ratio=-0.1), dict(ratio=1.5), dict(ratio=float("nan")),
                dict(ratio=None), dict(ratio="high"), dict(mx=0), dict(mx=-1.0), dict(mx=float("inf")), dict(mx=float("nan")), dict(mx=None),
                dict(seed=None), dict(epi=None), dict(epi=8196), dict(fast=True), dict(gray=True)):
        a = dict(x0_fix="dynamic", ratio=0.995, mx=1.0, seed=1, epi=EPI, fast=False, gray=False)
        a.update(bad)
        with pytest.raises(ValueError):
            check_x0_fix(a["x0_fix"], a["ratio"], a["mx"], seed=a["seed"], elems_per_image=a["epi"], fast_f32=a["fast"], gray=a["gray"])


def test_sampler_refusals_come_before_any_gpu_call(repo_root):
    """CifarNI on a device that need not exist: a bad correction argument is a ValueError from the host checks (without a GPU anything later is a
    RuntimeError)"""
    from naturaldiffusion_amd.coeff import load_coeff_npz
    C_, B_, node = load_coeff_npz(repo_root / "weights/step_5_weight_00.npz")
    for bad in (dict(x0_fix="static"), dict(x0_ratio=1.5), dict(x0_ratio=float("nan")), dict(x0_max=0.0), dict(x0_max=float("inf")),
                dict(fast_f32=True), dict(seed=None), dict(elems_per_image=8196, n=8196)):
        a = dict(x0_fix="dynamic", x0_ratio=0.995, x0_max=1.0, fast_f32=False, seed=1, elems_per_image=EPI, n=2 * EPI)
        a.update(bad)
        n = a.pop("n")
        with pytest.raises(ValueError):
            CifarNI(C_, B_, node, n, **a)
    for fn in (CifarNI.__init__, BatchLanes.__init__, generate_sharded, natural_inference_tx):
        p = inspect.signature(fn).parameters
        assert (p["x0_fix"].default, p["x0_ratio"].default, p["x0_max"].default) == (None, 0.995, 1.0), fn


def test_job_refusals_come_before_any_gpu_call(repo_root):
    """generate_sharded with a model that must never be called, on a device that need not exist"""
    w = repo_root / "weights/step_5_weight_00.npz"
    u8 = torch.zeros((6, 32, 32, 3), dtype=torch.uint8)
    m = torch.ones((6, 32, 32), dtype=torch.bool)

    def never(*a):
        raise AssertionError("the denoiser was called")
    for kw in (dict(x0_fix="static"), dict(x0_fix="dynamic", x0_ratio=1.01), dict(x0_fix="dynamic", x0_ratio=float("nan")),
               dict(x0_fix="clip", x0_max=0.0), dict(x0_fix="clip", x0_max=float("inf")), dict(x0_fix="dynamic", seed=None),
               dict(x0_fix="dynamic", gray=u8[..., 0]),                                       # colorization has no correction
               dict(x0_fix="dynamic", known=u8, mask=None), dict(x0_fix="clip", known=u8[:5], mask=m)):      # prepare_known's refusals still come first
        with pytest.raises(ValueError):
            generate_sharded(never, w, 6, 4, **kw)
    with pytest.raises(ValueError):
        BatchLanes([never], None, None, None, "cuda:0", seed=1, x0_fix="dynamic", x0_max=-1.0)
    with pytest.raises(ValueError):
        natural_inference_tx(batch_size=2, sample_count=2, x0_fix="dynamic", x0_ratio=2.0)
    # the preparation of the known pixels and of the gray picture is the same with or without a correction: pure host code
    assert prepare_known(u8, m, 6)[0].shape == (6, EPI) and prepare_gray(u8[..., 0], 6).shape == (6, 1024)
