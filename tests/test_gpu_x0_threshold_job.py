"""GPU tests of the CIFAR10 job with the x0 correction (generate_sharded(x0_fix=, x0_ratio=, x0_max=)): the thresholds the steps used are the
ones the denoiser was chosen to provoke, image i is the same bytes for any batch split or world size (the threshold is a per-image statistic),
and without the argument the job is the one it always was."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from naturaldiffusion_amd.coeff import load_coeff_npz

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
    """An elementwise denoiser, a function of (x, t) alone: out = c(t) * x / std(t), so that x0 = x * (1 - c * sigma^2 / std^2) / alpha.  Early steps
    (t > 0.5, c = 0): x0 = x / alpha, far over max_val = 1; late steps (c = 0.95): x0 ~ 0.05 x / alpha, under it."""
    t = labels / 999.0
    lmc = -0.25 * t ** 2 * (20.0 - 0.1) - 0.5 * t * 0.1
    std = torch.sqrt(1.0 - torch.exp(2.0 * lmc))
    c = torch.where(t > 0.5, torch.zeros_like(t), torch.full_like(t, 0.95))
    return x * (c / std)[:, None, None, None]


@pytest.mark.parametrize("matrix", ["det5", "sde18"])
def test_image_i_is_the_same_bytes_for_any_split_and_the_thresholds_are_of_both_kinds(dev, repo_root, matrix):
    from naturaldiffusion_amd.CIFAR10NaturalInference import BatchLanes, generate_sharded, philox_noise
    w = repo_root / MATRICES[matrix]
    kw = dict(x0_fix="dynamic", x0_ratio=0.995, x0_max=1.0)
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
    # the same batch through the lanes themselves, whose sampler keeps the thresholds of its last batch
    C, B, node = load_coeff_npz(w)
    lanes = BatchLanes([model_fn], C, B, node, dev, seed=SEED, **kw)
    lanes.submit(6, noise_fn=lambda: philox_noise(range(6), (3, 32, 32), SEED, dev), index=(0, 1))
    assert torch.equal(lanes.finish()[0].cpu(), b6)
    s = lanes.samplers[0][6].x0_s.cpu()
    assert tuple(s.shape) == (C.shape[0], 6) and s.dtype == torch.float64
    assert bool((s > 1.0).any()) and bool((s == 1.0).any()) and bool((s >= 1.0).all()), s
    assert bool((s[0] > 1.0).all()) and bool((s[-1] == 1.0).all())
    # the correction changes the images, and each mode its own way
    clip, _ = generate_sharded(model_fn, w, 6, 4, x0_fix="clip")
    plain, _ = generate_sharded(model_fn, w, 6, 4)
    assert not torch.equal(b6, plain) and not torch.equal(clip, plain) and not torch.equal(clip, b6)


@pytest.mark.parametrize("matrix", ["det5", "sde18"])
def test_x0_fix_none_is_the_job_without_the_argument(dev, repo_root, monkeypatch, matrix):
    from naturaldiffusion_amd import _lib
    from naturaldiffusion_amd.CIFAR10NaturalInference import generate_sharded

    def boom(*a):
        raise AssertionError("a correction entry was called")
    monkeypatch.setattr(_lib.lib, "natinf_step_f64hist_x0fix", boom)
    monkeypatch.setattr(_lib.lib, "natinf_x0_threshold_f64", boom)
    w = repo_root / MATRICES[matrix]
    plain, ip = generate_sharded(model_fn, w, 7, 3)
    none, inn = generate_sharded(model_fn, w, 7, 3, x0_fix=None, x0_ratio=0.5, x0_max=2.0)        # the other two are not looked at
    assert torch.equal(ip, inn) and torch.equal(none, plain)


def test_correction_goes_with_inpainting(dev, repo_root):
    """known pixels with the correction: the known pixels come back as given (known_final="data"), the job is split-invariant, and the rest of
    the image differs from the job without the correction"""
    import numpy as np
    from naturaldiffusion_amd.CIFAR10NaturalInference import generate_sharded
    w = repo_root / MATRICES["det5"]
    rs = np.random.RandomState(3)
    u8 = torch.from_numpy(rs.randint(0, 256, size=(6, 32, 32, 3)).astype(np.uint8))
    m = torch.zeros((6, 32, 32), dtype=torch.bool)
    m[:, :, :16] = True
    kw = dict(known=u8, mask=m, known_final="data")
    a, _ = generate_sharded(model_fn, w, 6, 6, x0_fix="dynamic", **kw)
    b, _ = generate_sharded(model_fn, w, 6, 4, x0_fix="dynamic", **kw)
    plain, _ = generate_sharded(model_fn, w, 6, 4, **kw)
    k = m[..., None].expand(-1, -1, -1, 3)
    assert torch.equal(a, b) and torch.equal(a[k], u8[k]) and torch.equal(plain[k], u8[k]) and not torch.equal(a[~k], plain[~k])
