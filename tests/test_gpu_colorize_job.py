"""GPU tests of the CIFAR10 colorization job (generate_sharded(gray=, known_final=)): the job is CifarNI.run(gray_u=) batch by batch, the gray
channel of its result is the gray picture at the last level, a shared picture equals the repeated one; with the NCSN++ engine image i is the same
bytes for any batch split or world size and differs from the unconditional one; without the new argument the job is the one it always was."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from naturaldiffusion_amd.coeff import load_coeff_npz
from oracle import ni_oracle as O

SEED = 888
ULP = 2.0 ** -24
MATRICES = {"det5": "weights/step_5_weight_00.npz", "sde18": "results/euler_heun/sde_euler_018.npz"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def gray_pictures(n, seed=0):
    """gray uint8 pictures [n, 32, 32]"""
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=(n, 32, 32)).astype(np.uint8))


# ------------------------------------------------------------------------------ 1. elementwise denoiser
@pytest.mark.parametrize("matrix", ["det5", "sde18"])
def test_job_is_the_sampler_run_batch_by_batch_and_its_gray_channel_the_picture(dev, repo_root, matrix):
    """The job's bytes == to_pixel_from_centered of CifarNI.run(gray_u=) per batch.  On run's float result latent channel 0 is fp32(alpha_N*gray_u)
    ("mean") or gray_u ("data"), and latent channels 1, 2 are those of the last step's unblended x_next, each within 16 * 2^-24 * s,
    s = max(1, |target|, max |M^T x|) with x that unblended x_next (tests/test_colorize_host.py has the derivation of the bound)."""
    from naturaldiffusion_amd.CIFAR10NaturalInference import (gather_known, generate_sharded, philox_noise, prepare_gray,
                                                              to_pixel_from_centered)
    from naturaldiffusion_amd.sampler import COLOR_M, CifarNI
    from naturaldiffusion_amd.shard import rank_batches
    w = repo_root / MATRICES[matrix]
    C, B, node = load_coeff_npz(w)
    N = C.shape[0]
    model = O.analytic_vp_model()
    n, bs = 6, 4
    g8 = gray_pictures(n)
    rows = prepare_gray(g8, n)
    plain, ip = generate_sharded(model, w, n, bs)
    M64 = COLOR_M.astype(np.float64)
    for final in ("mean", "data"):
        got, idx = generate_sharded(model, w, n, bs, gray=g8, known_final=final)
        assert torch.equal(idx, ip) and got.shape == plain.shape == (n, 32, 32, 3)
        assert not torch.equal(got, plain)
        alpha = np.float32(node[-1, 1]) if final == "mean" else np.float32(1.0)
        for b in rank_batches(n, bs, 0, 1):
            noise = philox_noise(b, (3, 32, 32), SEED, dev)
            ni = CifarNI(C, B, node, noise.numel(), device=dev, seed=SEED, elems_per_image=3072)
            gu = gather_known(rows, b).to(dev)
            xs = ni.run(model, noise, return_all=True, index=(b[0], 1), gray_u=gu, known_final=final)
            assert torch.equal(to_pixel_from_centered(xs[-1]), got[b]), (final, b)
            # the last step once more without the blend: its history is still in the sampler
            labels = torch.full((len(b),), ni.labels[N - 1], dtype=torch.float32, device=dev)
            args = (N - 1, xs[N - 1].reshape(-1), model(xs[N - 1], labels).contiguous().reshape(-1), noise.reshape(-1))
            un = (ni.step(*args, index=(b[0], 1)) if ni.stochastic else ni.step(*args)).cpu().numpy().astype(np.float64).reshape(len(b), 3, 1024)
            lat_in = np.einsum("nip,ij->njp", un, M64)
            lat_out = np.einsum("nip,ij->njp", xs[-1].cpu().numpy().astype(np.float64).reshape(len(b), 3, 1024), M64)
            target = (rows[b].numpy() * alpha).astype(np.float64)                          # fp32 product: std 0 at the last level
            s = np.maximum(1.0, np.maximum(np.abs(target), np.abs(lat_in).max(axis=1)))
            e0, e12 = np.abs(lat_out[:, 0] - target) / s, np.abs(lat_out[:, 1:] - lat_in[:, 1:]) / s[:, None]
            print(f"{matrix} {final} batch {b[0]}..: gray {e0.max() / ULP:.2f}, rest {e12.max() / ULP:.2f} ulp*s")
            assert (e0 <= 16 * ULP).all() and (e12 <= 16 * ULP).all()


def test_shared_picture_equals_the_repeated_one_and_a_gray_picture_its_expansion(dev, repo_root):
    from naturaldiffusion_amd.CIFAR10NaturalInference import generate_sharded
    w = repo_root / MATRICES["det5"]
    model = O.analytic_vp_model()
    n = 5
    g8 = gray_pictures(n, 1)
    rep, _ = generate_sharded(model, w, n, 2, gray=g8[:1].expand(n, -1, -1).contiguous())
    one, _ = generate_sharded(model, w, n, 2, gray=g8[:1])                                  # K = 1
    assert torch.equal(one, rep)
    per, _ = generate_sharded(model, w, n, 2, gray=g8)
    ggg, _ = generate_sharded(model, w, n, 2, gray=g8[..., None].expand(-1, -1, -1, 3).contiguous())
    assert torch.equal(per, ggg) and not torch.equal(per, rep)


# ------------------------------------------------------------------------------ 2. the real engine
@pytest.fixture(scope="module")
def engine_jobs(dev, repo_root):
    from naturaldiffusion_amd.CIFAR10NaturalInference import generate_sharded
    from naturaldiffusion_amd.ncsnpp import NCSNppEngine, flatten_state_dict
    from naturaldiffusion_amd.synth import synthetic_state_dict
    w = repo_root / MATRICES["det5"]
    eng = NCSNppEngine(flatten_state_dict(synthetic_state_dict(0)), max_batch=8, device=dev)
    kw = dict(gray=gray_pictures(8, 2))
    return dict(plain=generate_sharded(eng, w, 8, 8)[0],
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


def test_engine_every_image_differs_from_the_unconditional_one(engine_jobs):
    j = engine_jobs
    per_image = [(j["b8"][i] != j["plain"][i]).any().item() for i in range(8)]
    assert all(per_image), per_image


# ------------------------------------------------------------------------------ 3. no regression
@pytest.mark.parametrize("matrix", ["det5", "sde18"])
def test_without_gray_the_job_is_the_one_it_was(dev, repo_root, monkeypatch, matrix):
    """generate_sharded called as before == the loop it always ran (philox_noise, natural_inference, to_pixel_from_centered), and neither
    colorization entry is reached"""
    from naturaldiffusion_amd import _lib
    from naturaldiffusion_amd.CIFAR10NaturalInference import generate_sharded, natural_inference, philox_noise, to_pixel_from_centered
    from naturaldiffusion_amd.shard import rank_batches

    def boom(*a):
        raise AssertionError("a colorization entry was called")
    monkeypatch.setattr(_lib.lib, "natinf_color_blend_f32", boom)
    monkeypatch.setattr(_lib.lib, "natinf_step_f64hist_colorize", boom)
    w = repo_root / MATRICES[matrix]
    model = O.analytic_vp_model()
    got, idx = generate_sharded(model, w, 7, 3)
    assert torch.equal(idx, torch.arange(7))
    for b in rank_batches(7, 3, 0, 1):
        x = natural_inference(model, philox_noise(b, (3, 32, 32), SEED, dev), w, seed=SEED, first_index=b[0])
        assert torch.equal(to_pixel_from_centered(x), got[b]), b
