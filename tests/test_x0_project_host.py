"""Host pieces of the x0 projection of the CIFAR10 form (super-resolution; no GPU): the numpy mirror of the arithmetic contract against a plain
mean and against an explicit double loop in the defined order, the properties that make it a projection, the refusals of the two ABI entries,
which touch no device, and the refusals of the sampler and the job, which all come before any GPU call."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from naturaldiffusion_amd import _lib
from naturaldiffusion_amd.CIFAR10NaturalInference import (BatchLanes, downsample_images, generate_sharded, natural_inference_tx, prepare_lowres,
                                                          u8_to_centered)
from naturaldiffusion_amd.sampler import CifarNI, check_project, downsample_host, x0_project_host

lib = _lib.lib
EPI = 3 * 32 * 32
EINVAL = -1
QNAN = np.uint64(0x7FF8000000000000)
SHAPES = [(1, 2, 2, 2), (3, 2, 6, 2), (1, 8, 8, 8), (3, 8, 16, 4), (3, 32, 32, 2), (3, 32, 32, 4), (3, 32, 32, 8), (3, 32, 36, 4), (2, 64, 64, 8)]
SCALES = [0.05, 1.0, 1e3]


def _up(low, c, h, w, s):
    return np.repeat(np.repeat(low.reshape(-1, c, h // s, w // s), s, axis=2), s, axis=3).reshape(low.shape[0], -1)


def _loop_average(img, c, h, w, s):
    """A of one image with Python floats (IEEE doubles), written in the defined order"""
    out = np.empty((c, h // s, w // s))
    for ch in range(c):
        for bi in range(h // s):
            for bj in range(w // s):
                total = None
                for j in range(s):
                    row = float(img[ch, s * bi + j, s * bj])
                    for i in range(1, s):
                        row = row + float(img[ch, s * bi + j, s * bj + i])
                    total = row if total is None else total + row
                out[ch, bi, bj] = total * (1.0 / (s * s))
    return out.reshape(-1)


# ------------------------------------------------------------------------------ 1. the block average
@pytest.mark.parametrize("c,h,w,s", SHAPES)
def test_downsample_against_a_plain_mean_and_the_defined_order(c, h, w, s):
    rs = np.random.RandomState(c * h * w + s)
    x = rs.randn(3, c * h * w) * np.array([0.05, 1.0, 1e3])[:, None]
    got = downsample_host(x, (c, h, w), s)
    assert got.dtype == np.float64 and got.shape == (3, c * (h // s) * (w // s))
    mean = x.reshape(3, c, h // s, s, w // s, s).mean(axis=(3, 5)).reshape(3, -1)
    blocks = np.abs(x).reshape(3, c, h // s, s, w // s, s).max(axis=(3, 5)).reshape(3, -1)
    assert (np.abs(got - mean) <= 4 * np.spacing(blocks)).all()                 # 4 ulp of the block's largest element
    for i in range(3 if c * h * w <= 3072 else 1):                               # (the double loop is slow: one image of the largest shapes)
        want = _loop_average(x[i].reshape(c, h, w), c, h, w, s)
        assert np.array_equal(got[i].view(np.uint64), want.view(np.uint64)), (c, h, w, s, i)
    one = downsample_host(x[0], (c, h, w), s)                                    # one flat image
    assert one.shape == got[0].shape and np.array_equal(one, got[0])
    assert np.array_equal(downsample_host(x.reshape(3, c, h, w), (c, h, w), s), got)


def test_no_zero_seed_keeps_the_sign_of_zero():
    x = np.full((1, 4), -0.0)
    assert np.signbit(downsample_host(x, (1, 2, 2), 2)).all()


# ------------------------------------------------------------------------------ 2. the projection
@pytest.mark.parametrize("c,h,w,s", SHAPES)
@pytest.mark.parametrize("scale", SCALES)
def test_projection_properties(c, h, w, s, scale):
    """With M = max(|x|, |y|, |low|) of the image: |A y - low| <= (2 s^2 + 2) 2^-53 M (s^2 - 1 additions in A y, its product, the subtraction and the
    addition that made y, each half an ulp of at most M, and as many again for the A x inside d); |A fp32(y) - low| <= 2^-23 M (fp32 rounding moves
    every element by at most 2^-24 M, and so the mean; the fp64 bound is far below the other 2^-24 M); the high-frequency part y - up(A y) is that of x."""
    rs = np.random.RandomState(c * h * w + s)
    n = 4
    x = rs.randn(n, c * h * w) * scale
    low = rs.randn(n, c * (h // s) * (w // s)) * scale
    for lo in (low, low[:1]):                                                    # one row per image; one shared row
        y, r = x0_project_host(x, lo, (c, h, w), s)
        lo_n = np.broadcast_to(lo, low.shape)
        assert y.dtype == np.float64 and y.shape == x.shape and r.shape == (n,)
        M = np.maximum(np.maximum(np.abs(x).max(1), np.abs(y).max(1)), np.abs(lo_n).max(1))[:, None]
        b64 = (2 * s * s + 2) * 2.0 ** -53 * M
        assert (np.abs(downsample_host(y, (c, h, w), s) - lo_n) <= b64).all()
        y32 = y.astype(np.float32).astype(np.float64)
        assert (np.abs(downsample_host(y32, (c, h, w), s) - lo_n) <= 2.0 ** -23 * M).all()
        hf_y = y - _up(downsample_host(y, (c, h, w), s), c, h, w, s)
        hf_x = x - _up(downsample_host(x, (c, h, w), s), c, h, w, s)
        assert (np.abs(hf_y - hf_x) <= b64).all()
        d = lo_n - downsample_host(x, (c, h, w), s)
        assert np.array_equal(r, np.abs(d).max(1))
        assert np.array_equal(y, x + _up(d, c, h, w, s))
    one, r1 = x0_project_host(x[0], low[0], (c, h, w), s)                        # one flat image
    assert one.shape == (c * h * w,) and r1.shape == (1,) and np.array_equal(one, x0_project_host(x, low, (c, h, w), s)[0][0])


@pytest.mark.parametrize("c,h,w,s", [(3, 8, 16, 4), (3, 2, 6, 2), (1, 8, 8, 8), (3, 32, 32, 4)])
def test_a_nan_or_an_inf_stays_in_its_block(c, h, w, s):
    rs = np.random.RandomState(5)
    x = rs.randn(3, c * h * w)
    low = rs.randn(3, c * (h // s) * (w // s))
    clean, _ = x0_project_host(x, low, (c, h, w), s)
    owner = _up(np.arange(c * (h // s) * (w // s), dtype=np.float64)[None], c, h, w, s)[0].astype(np.int64)      # element -> its block
    # a NaN in one element of image 1
    xn = x.copy()
    e = c * h * w // 2 + 1
    xn[1, e] = -np.nan
    y, r = x0_project_host(xn, low, (c, h, w), s)
    hit = owner == owner[e]
    assert np.isnan(y[1, hit]).all() and (y[1, hit].view(np.uint64) == QNAN).all()
    assert np.array_equal(y[1, ~hit], clean[1, ~hit]) and np.array_equal(y[[0, 2]], clean[[0, 2]])
    assert np.isnan(r[1]) and r[1:2].view(np.uint64)[0] == QNAN and np.isfinite(r[[0, 2]]).all()
    # an inf in one value of low of image 2
    li = low.copy()
    b = low.shape[1] - 1
    li[2, b] = np.inf
    y, r = x0_project_host(x, li, (c, h, w), s)
    hit = owner == b
    assert np.isposinf(y[2, hit]).all() and np.array_equal(y[2, ~hit], clean[2, ~hit]) and np.array_equal(y[:2], clean[:2])
    assert np.isposinf(r[2]) and np.isfinite(r[:2]).all()
    # inf in x and in low of the same block: inf - inf, the block is NaN and no other
    xi = x.copy()
    xi[2, np.flatnonzero(hit)[0]] = np.inf
    y, r = x0_project_host(xi, li, (c, h, w), s)
    assert (y[2, hit].view(np.uint64) == QNAN).all() and np.array_equal(y[2, ~hit], clean[2, ~hit]) and np.isnan(r[2])


def test_mirror_refuses_bad_geometry():
    x = np.zeros((1, 48))
    for shape, s in (((3, 4, 4), 3), ((3, 4, 4), 16), ((3, 4, 4), 8), ((3, 6, 4), 4), ((3, 4, 6), 4), ((0, 4, 4), 2), ((3, 4), 2), ((1, 2, 7), 2),
                     ((3, 64, 64), 2), ((3, 4, 4), 2.0), ((3, 4, 4), True)):
        with pytest.raises(ValueError):
            downsample_host(x, shape, s)
    with pytest.raises(ValueError):
        downsample_host(np.zeros(40), (3, 4, 4), 2)
    with pytest.raises(ValueError):
        x0_project_host(np.zeros((3, 48)), np.zeros((2, 12)), (3, 4, 4), 2)


# ------------------------------------------------------------------------------ 3. the ABI: exported, signed, and every refusal without a device
def test_library_exports_and_signs_both_entries():
    for name, n_args in (("natinf_x0_project_f64", 10), ("natinf_step_f64hist_project", 30)):
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        assert res is C.c_int and len(args) == n_args and fn.restype is C.c_int and list(fn.argtypes) == list(args)
    noise = _lib.SIGNATURES["natinf_step_f64hist_noise"][1]
    proj = _lib.SIGNATURES["natinf_step_f64hist_project"][1]
    assert list(proj) == list(noise[:-1]) + [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]


P = 4096                                                                     # a dummy non-NULL, 16-byte aligned address: no refused call reads it


def _project(**kw):
    a = dict(x0=P, low=P, r_out=P, n_images=3, c=3, h=32, w=32, s=4, ls=192)
    a.update(kw)
    return lib.natinf_x0_project_f64(a["x0"], a["low"], a["r_out"], a["n_images"], a["c"], a["h"], a["w"], a["s"], a["ls"], None)


def _step(**kw):
    a = dict(x_k=P, model_out=P, noise=P, hist=P, x_next=P, idx=P, val=P, n_terms=2, c_diag=1.0, idx_b=P, val_b=P, n_b=1, k=2, alpha=0.9,
             sigma=0.4, std=0.4, seed=7, index=None, first=0, stride=1, epi=EPI, E=3 * EPI, low=P, ls=192, c=3, h=32, w=32, s=4, r_out=None)
    a.update(kw)
    return lib.natinf_step_f64hist_project(a["x_k"], a["model_out"], a["noise"], a["hist"], a["x_next"], a["idx"], a["val"], a["n_terms"],
                                           a["c_diag"], a["idx_b"], a["val_b"], a["n_b"], a["k"], a["alpha"], a["sigma"], a["std"], a["seed"],
                                           a["index"], a["first"], a["stride"], a["epi"], a["E"], a["low"], a["ls"], a["c"], a["h"], a["w"],
                                           a["s"], a["r_out"], None)


BAD_GEOMETRY = [dict(low=None), dict(s=0), dict(s=1), dict(s=3), dict(s=16), dict(s=-2), dict(c=0), dict(c=-3), dict(h=0), dict(h=-32), dict(w=0),
                dict(w=-32), dict(s=8, h=36, ls=0), dict(s=8, w=36, ls=0), dict(h=30, ls=0), dict(w=30, ls=0), dict(ls=191), dict(ls=EPI),
                dict(ls=768), dict(ls=-192), dict(s=2, ls=192)]


def test_project_entry_refusals_touch_no_device():
    """(height and width multiples of s >= 2 make channels*height*width a multiple of 4, so that refusal is reachable through the step entry only)"""
    for bad in BAD_GEOMETRY + [dict(x0=None), dict(n_images=0), dict(n_images=-2),
                               dict(c=3, h=64, w=64, s=2, ls=0),                   # 12,288 elements: over the cap
                               dict(c=2, h=64, w=66, s=2, ls=0),                   # 8,448: just over
                               dict(c=2 ** 20, h=2 ** 20, w=2 ** 20, s=2, ls=0),   # a product past 2^32 must not pass either
                               dict(c=1, h=2, w=6, s=2, ls=2)]:                    # stride 2 for an image of 3 blocks
        assert _project(**bad) == EINVAL, bad


def test_step_entry_refusals_touch_no_device():
    for bad in BAD_GEOMETRY:
        assert _step(**bad) == EINVAL, bad
    # every refusal natinf_step_f64hist_noise makes for its own arguments
    for bad in (dict(x_k=None), dict(model_out=None), dict(noise=None), dict(hist=None), dict(x_next=None), dict(idx=None), dict(val=None),
                dict(n_terms=-1), dict(idx_b=None), dict(val_b=None), dict(n_b=-1), dict(k=-1), dict(E=0), dict(E=3 * EPI + 2), dict(epi=0),
                dict(epi=EPI, E=EPI + 4), dict(epi=6, E=24)):
        assert _step(**bad) == EINVAL, bad
    # the shape must be the image: channels*height*width == elems_per_image, at most 8192
    for bad in (dict(epi=EPI // 3, E=EPI), dict(c=1), dict(c=6), dict(h=16, ls=0), dict(w=16, ls=0),
                dict(c=3, h=64, w=64, s=4, ls=0, epi=12288, E=12288), dict(c=2, h=64, w=66, s=2, ls=0, epi=8448, E=8448)):
        assert _step(**bad) == EINVAL, bad


# ------------------------------------------------------------------------------ 4. the sampler and the job refuse on the host
GOOD = dict(sr_scale=4, shape=(3, 32, 32), seed=1, epi=EPI, fast=False, x0_fix=None, conditioned=False)


def test_check_project():
    assert check_project(None, "x", seed=None, elems_per_image=None) == 0    # no projection: nothing else is looked at
    assert [check_project(s, (3, 32, 32), seed=1, elems_per_image=EPI) for s in (2, 4, 8)] == [2, 4, 8]
    assert check_project(2, (3, 2, 6), seed=0, elems_per_image=36) == 2 and check_project(8, (2, 64, 64), seed=0, elems_per_image=8192) == 8
    assert check_project(4, (3, 32, 32), seed=1, elems_per_image=None, epi_later=True) == 4
    for bad in (dict(sr_scale=3), dict(sr_scale=16), dict(sr_scale=0), dict(sr_scale="4"), dict(sr_scale=4.0), dict(sr_scale=True),
                dict(shape=None), dict(shape=(32, 32)), dict(shape=(3, 32, 30)), dict(shape=(3, 30, 32)), dict(shape=(0, 32, 32)),
                dict(shape=(3, -32, 32)), dict(shape=(3, 32.0, 32)), dict(shape=(3, 64, 64), epi=12288), dict(shape=(3, 16, 16)),
                dict(fast=True), dict(x0_fix="clip"), dict(x0_fix="dynamic"), dict(conditioned=True), dict(seed=None), dict(epi=None),
                dict(epi=EPI + 4)):
        a = dict(GOOD, **bad)
        with pytest.raises(ValueError):
            check_project(a["sr_scale"], a["shape"], seed=a["seed"], elems_per_image=a["epi"], fast_f32=a["fast"], x0_fix=a["x0_fix"],
                          conditioned=a["conditioned"])


def test_sampler_refusals_come_before_any_gpu_call(repo_root):
    """CifarNI on a device that need not exist: a bad projection argument is a ValueError from the host checks (without a GPU anything later is a
    RuntimeError)"""
    from naturaldiffusion_amd.coeff import load_coeff_npz
    C_, B_, node = load_coeff_npz(repo_root / "weights/step_5_weight_00.npz")
    for bad in (dict(sr_scale=3), dict(image_shape=None), dict(image_shape=(3, 32, 30)), dict(fast_f32=True), dict(seed=None), dict(x0_fix="clip"),
                dict(x0_fix="dynamic"), dict(elems_per_image=1024), dict(image_shape=(3, 64, 64), elems_per_image=12288, n=12288)):
        a = dict(sr_scale=4, image_shape=(3, 32, 32), fast_f32=False, seed=1, elems_per_image=EPI, n=2 * EPI)
        a.update(bad)
        n = a.pop("n")
        with pytest.raises(ValueError):
            CifarNI(C_, B_, node, n, **a)
    for fn in (CifarNI.__init__, BatchLanes.__init__, generate_sharded, natural_inference_tx):
        assert inspect.signature(fn).parameters["sr_scale"].default is None, fn
    assert inspect.signature(CifarNI.__init__).parameters["image_shape"].default is None
    for fn in (CifarNI.step, CifarNI.run, BatchLanes.submit):
        assert inspect.signature(fn).parameters["low"].default is None, fn
    for fn in (CifarNI.run, BatchLanes.submit, generate_sharded, natural_inference_tx):
        assert inspect.signature(fn).parameters["sr_final"].default == "step", fn
    for fn in (generate_sharded, natural_inference_tx):
        assert inspect.signature(fn).parameters["lowres"].default is None, fn


def test_prepare_lowres_and_downsample_images():
    rs = np.random.RandomState(2)
    u8 = torch.from_numpy(rs.randint(0, 256, size=(5, 32, 32, 3)).astype(np.uint8))
    f32 = u8_to_centered(u8.permute(0, 3, 1, 2))
    for s in (2, 4, 8):
        n = 32 // s
        low = downsample_images(u8, s)
        assert low.dtype == torch.float64 and tuple(low.shape) == (5, 3 * n * n) and torch.equal(low, downsample_images(f32, s))
        want = downsample_host(f32.numpy().astype(np.float64).reshape(5, -1), (3, 32, 32), s)
        assert np.array_equal(low.numpy(), want)
        rows = prepare_lowres(low.reshape(5, 3, n, n), s, 5)                     # fp64 rows go through as they are
        assert rows.dtype == torch.float64 and rows.device.type == "cpu" and torch.equal(rows, low)
        assert torch.equal(prepare_lowres(low.reshape(5, 3, n, n).float(), s, 5), low.float().double())
        assert tuple(prepare_lowres(low[:1].reshape(1, 3, n, n), s, 5).shape) == (1, 3 * n * n)      # one shared row
        small = torch.from_numpy(rs.randint(0, 256, size=(5, n, n, 3)).astype(np.uint8))
        assert torch.equal(prepare_lowres(small, s, 5), u8_to_centered(small.permute(0, 3, 1, 2)).double().reshape(5, -1))
        for bad in (low, low.reshape(5, n, n, 3), low[:4].reshape(4, 3, n, n), small[:3], small.permute(0, 3, 1, 2), low.reshape(5, 3, n, n).half()):
            with pytest.raises(ValueError):
                prepare_lowres(bad, s, 5)
    for bad in (u8[:, :16], f32.double(), f32.permute(0, 2, 3, 1), u8.permute(0, 3, 1, 2)):
        with pytest.raises(ValueError):
            downsample_images(bad, 4)
    with pytest.raises(ValueError):
        downsample_images(u8, 3)
    with pytest.raises(ValueError):
        prepare_lowres(low, 5, 5)


def test_job_refusals_come_before_any_gpu_call(repo_root):
    """generate_sharded with a model that must never be called, on a device that need not exist"""
    w = repo_root / "weights/step_5_weight_00.npz"
    u8 = torch.zeros((6, 32, 32, 3), dtype=torch.uint8)
    m = torch.ones((6, 32, 32), dtype=torch.bool)
    low = downsample_images(u8, 4).reshape(6, 3, 8, 8)

    def never(*a):
        raise AssertionError("the denoiser was called")
    for kw in (dict(lowres=low), dict(sr_scale=4), dict(lowres=low, sr_scale=3), dict(lowres=low, sr_scale=2), dict(lowres=low[:5], sr_scale=4),
               dict(lowres=low.reshape(6, -1), sr_scale=4), dict(lowres=low, sr_scale=4, sr_final="mean"), dict(sr_final="x0"),
               dict(lowres=low, sr_scale=4, seed=None), dict(lowres=low, sr_scale=4, x0_fix="clip"), dict(lowres=low, sr_scale=4, x0_fix="dynamic"),
               dict(lowres=low, sr_scale=4, known=u8, mask=m), dict(lowres=low, sr_scale=4, gray=u8[..., 0])):
        with pytest.raises(ValueError):
            generate_sharded(never, w, 6, 4, **kw)
    for kw in (dict(sr_scale=5), dict(sr_scale=4, x0_fix="clip"), dict(sr_scale=4, seed=None)):
        with pytest.raises(ValueError):
            BatchLanes([never], None, None, None, "cuda:0", **dict(dict(seed=1), **kw))
    for kw in (dict(lowres=low[:2]), dict(lowres=low[:2], sr_scale=16), dict(lowres=low[:3], sr_scale=4), dict(lowres=low[:2], sr_scale=4, sr_final="last"),
               dict(lowres=low[:2], sr_scale=4, x0_fix="clip")):
        with pytest.raises(ValueError):
            natural_inference_tx(batch_size=2, sample_count=2, **kw)
