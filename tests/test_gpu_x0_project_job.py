"""GPU tests of the CIFAR10 job with the x0 projection (generate_sharded(lowres=, sr_scale=, sr_final=)): image i is the same bytes for any
batch split or world size (the projection is a function of the image's own x0 and its own row of lowres), without the arguments the job is the
one it always was, and with the ideal denoiser of a small training set the job does super-resolution: every image generated from the block
averages of a training picture lands on that picture."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from naturaldiffusion_amd import coeffgen as G

SEED = 888
MATRICES = {"det5": "weights/step_5_weight_00.npz", "sde18": "results/euler_heun/sde_euler_018.npz"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def model_fn(x, labels):
    """An elementwise denoiser, a function of (x, t) alone: out = c(t) * x / std(t) (tests/test_gpu_x0_threshold_job.py)"""
    t = labels / 999.0
    lmc = -0.25 * t ** 2 * (20.0 - 0.1) - 0.5 * t * 0.1
    std = torch.sqrt(1.0 - torch.exp(2.0 * lmc))
    c = torch.where(t > 0.5, torch.zeros_like(t), torch.full_like(t, 0.95))
    return x * (c / std)[:, None, None, None]


@pytest.mark.parametrize("matrix", ["det5", "sde18"])
@pytest.mark.parametrize("shared", [False, True])
def test_image_i_is_the_same_bytes_for_any_split(dev, repo_root, matrix, shared):
    from naturaldiffusion_amd.CIFAR10NaturalInference import BatchLanes, generate_sharded, philox_noise
    from naturaldiffusion_amd.coeff import load_coeff_npz
    w = repo_root / MATRICES[matrix]
    rs = np.random.RandomState(4)
    lowres = torch.from_numpy(rs.uniform(-1, 1, size=(1 if shared else 6, 3, 8, 8)))
    kw = dict(lowres=lowres, sr_scale=4, sr_final="x0")
    b6, idx = generate_sharded(model_fn, w, 6, 6, **kw)
    assert b6.shape == (6, 32, 32, 3) and torch.equal(idx, torch.arange(6))
    b42, _ = generate_sharded(model_fn, w, 6, 4, **kw)
    assert torch.equal(b42, b6)
    full = torch.empty_like(b6)
    for r in range(2):
        im, ix = generate_sharded(model_fn, w, 6, 6, rank=r, world=2, **kw)
        assert im.shape[0] == 3 and ix.tolist() == [r, r + 2, r + 4]
        full[ix] = im
    assert torch.equal(full, b6)
    # the same batch through the lanes themselves, whose sampler keeps the residuals of its last batch
    C, B, node = load_coeff_npz(w)
    lanes = BatchLanes([model_fn], C, B, node, dev, seed=SEED, sr_scale=4)
    low = lowres.reshape(lowres.shape[0], -1).reshape(-1).to(dev)
    lanes.submit(6, noise_fn=lambda: philox_noise(range(6), (3, 32, 32), SEED, dev), index=(0, 1), low=low, sr_final="x0")
    assert torch.equal(lanes.finish()[0].cpu(), b6)
    r = lanes.samplers[0][6].sr_r.cpu()
    assert tuple(r.shape) == (C.shape[0], 6) and r.dtype == torch.float64 and bool((r > 0).all()) and bool(torch.isfinite(r).all())
    # the result the other way, and the job without the projection: three different sets of images
    step, _ = generate_sharded(model_fn, w, 6, 4, lowres=lowres, sr_scale=4)
    plain, _ = generate_sharded(model_fn, w, 6, 4)
    assert not torch.equal(b6, plain) and not torch.equal(step, plain) and not torch.equal(step, b6)


@pytest.mark.parametrize("matrix", ["det5", "sde18"])
def test_lowres_none_is_the_job_without_the_argument(dev, repo_root, monkeypatch, matrix):
    from naturaldiffusion_amd import _lib
    from naturaldiffusion_amd.CIFAR10NaturalInference import generate_sharded

    def boom(*a):
        raise AssertionError("a projection entry was called")
    monkeypatch.setattr(_lib.lib, "natinf_step_f64hist_project", boom)
    monkeypatch.setattr(_lib.lib, "natinf_x0_project_f64", boom)
    w = repo_root / MATRICES[matrix]
    plain, ip = generate_sharded(model_fn, w, 7, 3)
    none, inn = generate_sharded(model_fn, w, 7, 3, lowres=None, sr_scale=None, sr_final="step")
    assert torch.equal(ip, inn) and torch.equal(none, plain)


def training_pictures():
    """8 synthetic 32 x 32 pictures: 0.7 up4(uniform[-1, 1] at 8 x 8) + 0.3 uniform[-1, 1], clipped to [-1, 1] -> uint8 [8, 32, 32, 3]"""
    rs = np.random.RandomState(0)
    coarse = rs.uniform(-1, 1, size=(8, 3, 8, 8))
    fine = rs.uniform(-1, 1, size=(8, 3, 32, 32))
    pic = np.clip(0.7 * np.repeat(np.repeat(coarse, 4, 2), 4, 3) + 0.3 * fine, -1, 1)
    u8 = np.clip(np.floor((pic + 1) / 2 * 255), 0, 255).astype(np.uint8)
    return torch.from_numpy(u8).permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def ideal(dev):
    from naturaldiffusion_amd.CIFAR10NaturalInference import ideal_denoiser
    train = training_pictures()
    return train, ideal_denoiser(train, device=dev), G.ddim_vp_continuous(G.quadratic_time_grid(5))


@pytest.mark.parametrize("s", [2, 4])
def test_it_does_super_resolution(dev, ideal, s):
    """6 images per training picture t, each from the s x s block averages of picture t, a 5-step DDIM matrix, sr_final="x0": every one of the 48
    has picture t as its nearest training picture.  (A replay of this case on the CPU with x0_project_host gave 48 / 48 at s = 2 and s = 4, and 17 /
    48 at s = 8 -- 4 x 4 values of data --, which is therefore not asserted.)"""
    from naturaldiffusion_amd.CIFAR10NaturalInference import calc_nearest, downsample_images, generate_sharded
    train, den, coeff = ideal
    target = torch.arange(8).repeat_interleave(6)
    lowres = downsample_images(train, s)[target].reshape(48, 3, 32 // s, 32 // s)
    imgs, idx = generate_sharded(den, None, 48, 48, coeff=coeff, lowres=lowres, sr_scale=s, sr_final="x0")
    assert torch.equal(idx, torch.arange(48))
    near = calc_nearest(imgs, train, dev, space="pixel")["idx"][:, 0]
    assert near.tolist() == target.tolist(), (s, near.reshape(8, 6))


def test_without_the_projection_it_does_not(dev, ideal):
    from naturaldiffusion_amd.CIFAR10NaturalInference import calc_nearest, generate_sharded
    train, den, coeff = ideal
    target = torch.arange(8).repeat_interleave(6)
    imgs, _ = generate_sharded(den, None, 48, 48, coeff=coeff)
    near = calc_nearest(imgs, train, dev, space="pixel")["idx"][:, 0]
    assert (near != target.numpy()).any(), near.reshape(8, 6)
