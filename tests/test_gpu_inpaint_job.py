"""GPU tests of the CIFAR10 inpainting job (generate_sharded(known=, mask=, known_final=)): with an elementwise denoiser the unknown pixels
are those of the unconditional job and the known ones the final blend; with the NCSN++ engine the conditioning reaches the rest of the image
and image i is the same bytes for any batch split or world size; without the new arguments the job is the one it always was."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from naturaldiffusion_amd.coeff import load_coeff_npz
from oracle import ni_oracle as O

SEED = 888
MATRICES = {"det5": "weights/step_5_weight_00.npz", "sde18": "results/euler_heun/sde_euler_018.npz"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def picture(n, seed=0):
    """known uint8 images [n, 32, 32, 3] and the left-half pixel mask [n, 32, 32] plus a few scattered pixels per image"""
    rs = np.random.RandomState(seed)
    u8 = torch.from_numpy(rs.randint(0, 256, size=(n, 32, 32, 3)).astype(np.uint8))
    m = torch.zeros((n, 32, 32), dtype=torch.bool)
    m[:, :, :16] = True
    m |= torch.from_numpy(rs.rand(n, 32, 32) < 0.02)
    return u8, m


def nhwc(m):
    return m[..., None].expand(-1, -1, -1, 3)


# ------------------------------------------------------------------------------ 1. elementwise denoiser
@pytest.mark.parametrize("matrix", ["det5", "sde18"])
def test_elementwise_denoiser_unknown_pixels_unconditional_known_pixels_the_final_blend(dev, repo_root, matrix):
    from naturaldiffusion_amd.CIFAR10NaturalInference import generate_sharded, u8_to_centered
    w = repo_root / MATRICES[matrix]
    _, _, node = load_coeff_npz(w)
    model = O.analytic_vp_model()
    n = 6
    u8, m = picture(n)
    plain, ip = generate_sharded(model, w, n, 4)
    mean, im = generate_sharded(model, w, n, 4, known=u8, mask=m)
    data, _ = generate_sharded(model, w, n, 4, known=u8, mask=m, known_final="data")
    assert torch.equal(ip, im) and mean.shape == plain.shape == (n, 32, 32, 3)
    k = nhwc(m)
    assert torch.equal(mean[~k], plain[~k]) and torch.equal(data[~k], plain[~k])           # the model is elementwise: nothing reaches the rest
    alpha = float(np.float32(node[-1, 1]))
    want = O.to_pixel(u8_to_centered(u8.permute(0, 3, 1, 2)) * alpha)                      # std 0 at the last level: fp32(known*alpha_N)
    assert torch.equal(mean[k], want[k])
    assert torch.equal(data[k], u8[k])                                                     # the pixels as given, all of them
    assert not torch.equal(plain[k], u8[k])


def test_shared_mask_and_shared_picture_equal_the_repeated_ones(dev, repo_root):
    from naturaldiffusion_amd.CIFAR10NaturalInference import generate_sharded
    w = repo_root / MATRICES["det5"]
    model = O.analytic_vp_model()
    n = 5
    u8, m = picture(n, 1)
    rep, _ = generate_sharded(model, w, n, 2, known=u8, mask=m[:1].expand(n, -1, -1).contiguous())
    one, _ = generate_sharded(model, w, n, 2, known=u8, mask=m[:1])
    assert torch.equal(one, rep)
    rep, _ = generate_sharded(model, w, n, 2, known=u8[:1].expand(n, -1, -1, -1).contiguous(), mask=nhwc(m).permute(0, 3, 1, 2).contiguous())
    one, _ = generate_sharded(model, w, n, 2, known=u8[:1], mask=m)                        # [K', 32, 32] == its broadcast over the channels
    assert torch.equal(one, rep)


# ------------------------------------------------------------------------------ 2. the real engine
@pytest.fixture(scope="module")
def engine_jobs(dev, repo_root):
    from naturaldiffusion_amd.CIFAR10NaturalInference import generate_sharded
    from naturaldiffusion_amd.ncsnpp import NCSNppEngine, flatten_state_dict
    from naturaldiffusion_amd.synth import synthetic_state_dict
    w = repo_root / MATRICES["det5"]
    eng = NCSNppEngine(flatten_state_dict(synthetic_state_dict(0)), max_batch=8, device=dev)
    u8, m = picture(8, 2)
    kw = dict(known=u8, mask=m)
    return dict(u8=u8, m=m, eng=eng, w=w,
                plain=generate_sharded(eng, w, 8, 8)[0],
                b8=generate_sharded(eng, w, 8, 8, **kw)[0],
                b3=generate_sharded(eng, w, 8, 3, **kw)[0],
                halves=[generate_sharded(eng, w, 8, 8, rank=r, world=2, **kw) for r in range(2)])


def test_engine_image_i_is_the_same_bytes_for_any_split(engine_jobs):
    j = engine_jobs
    assert torch.equal(j["b8"], j["b3"])
    full = torch.empty_like(j["b8"])
    for im, ix in j["halves"]:
        assert im.shape[0] == 4
        full[ix] = im
    assert torch.equal(full, j["b8"])


def test_engine_conditioning_reaches_the_rest_of_the_image(engine_jobs):
    j = engine_jobs
    k = nhwc(j["m"])
    assert not torch.equal(j["b8"][~k], j["plain"][~k])
    per_image = [(j["b8"][i][~k[i]] != j["plain"][i][~k[i]]).any().item() for i in range(8)]
    assert all(per_image), per_image


# ------------------------------------------------------------------------------ 3. no regression
@pytest.mark.parametrize("matrix", ["det5", "sde18"])
def test_without_the_new_arguments_the_job_is_the_one_it_was(dev, repo_root, monkeypatch, matrix):
    """generate_sharded called as before == the loop it always ran (philox_noise, natural_inference, to_pixel_from_centered), and neither
    inpainting entry is reached"""
    from naturaldiffusion_amd import _lib
    from naturaldiffusion_amd.CIFAR10NaturalInference import generate_sharded, natural_inference, philox_noise, to_pixel_from_centered
    from naturaldiffusion_amd.shard import rank_batches

    def boom(*a):
        raise AssertionError("an inpainting entry was called")
    monkeypatch.setattr(_lib.lib, "natinf_known_blend_f32", boom)
    monkeypatch.setattr(_lib.lib, "natinf_step_f64hist_inpaint", boom)
    w = repo_root / MATRICES[matrix]
    model = O.analytic_vp_model()
    got, idx = generate_sharded(model, w, 7, 3)
    assert torch.equal(idx, torch.arange(7))
    for b in rank_batches(7, 3, 0, 1):
        x = natural_inference(model, philox_noise(b, (3, 32, 32), SEED, dev), w, seed=SEED, first_index=b[0])
        assert torch.equal(to_pixel_from_centered(x), got[b]), b
