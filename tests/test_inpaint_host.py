"""Host pieces of CIFAR10 inpainting (no GPU): the uint8 -> centred float map, the per-batch gathering of the known pixels by global image
index, the level and column schedule of the blend, and the refusals, which all come before any GPU call."""
import numpy as np
import pytest
import torch

from naturaldiffusion_amd.CIFAR10NaturalInference import gather_known, generate_sharded, prepare_known, u8_to_centered
from naturaldiffusion_amd.coeff import load_coeff_npz
from naturaldiffusion_amd.sampler import KNOWN_COLUMN0, check_known, known_schedule
from naturaldiffusion_amd.shard import rank_batches
from oracle import ni_oracle as O

EPI = 3 * 32 * 32


# ------------------------------------------------------------------------------ 1. the pixel map
def test_all_256_values_survive_the_round_trip():
    v = torch.arange(256, dtype=torch.uint8)
    x = u8_to_centered(v)
    assert x.dtype == torch.float32 and float(x.min()) > -1.0 and float(x.max()) == float(np.float32(1.0 + 1.0 / 255))     # 255 sits half a level above 1 and comes back through the clamp
    assert torch.equal(O.to_pixel(x.view(1, 1, 16, 16)).reshape(-1), v)
    # the kernel's own order of fp32 operations (k_to_pixel: (v + 1)/2, *255, clamp, truncate)
    y = (x.numpy() + np.float32(1.0)) / np.float32(2.0) * np.float32(255.0)
    assert y.dtype == np.float32 and np.array_equal(np.clip(y, 0, 255).astype(np.uint8), v.numpy())
    # half a level from either neighbour: no rounding of the job's can move a pixel
    assert np.abs(y - (np.arange(256) + 0.5)).max() < 1e-3


def test_prepare_known_formats():
    rs = np.random.RandomState(0)
    u8 = torch.from_numpy(rs.randint(0, 256, size=(5, 32, 32, 3)).astype(np.uint8))
    m2 = torch.from_numpy(rs.rand(5, 32, 32) < 0.5)
    kf, mk = prepare_known(u8, m2, 5)
    assert kf.shape == (5, EPI) and kf.dtype == torch.float32 and mk.shape == (5, EPI) and mk.dtype == torch.uint8
    assert torch.equal(O.to_pixel(kf.view(5, 3, 32, 32)), u8)                             # NCHW, centred, exact
    assert torch.equal(mk.view(5, 3, 32, 32), m2[:, None].expand(-1, 3, -1, -1).to(torch.uint8))
    f32 = torch.from_numpy(rs.randn(1, 3, 32, 32).astype(np.float32))
    m4 = torch.from_numpy((rs.rand(1, 3, 32, 32) < 0.5).astype(np.uint8) * 255)           # any non-zero byte = known
    kf, mk = prepare_known(f32, m4, 5)
    assert kf.shape == (1, EPI) and torch.equal(kf.view(1, 3, 32, 32), f32)
    assert mk.shape == (1, EPI) and set(mk.unique().tolist()) <= {0, 1} and torch.equal(mk.view(1, 3, 32, 32) != 0, m4 != 0)


# ------------------------------------------------------------------------------ 2. gathering by global index
@pytest.mark.parametrize("count,batch,world", [(11, 4, 1), (11, 3, 2), (7, 8, 3), (5, 1, 5)])
def test_gather_by_global_index(count, batch, world):
    rows = torch.arange(count * 8, dtype=torch.float32).view(count, 8)                      # row i is recognisable as image i
    one = torch.full((1, 8), 7.0)
    seen = []
    for rank in range(world):
        for b in rank_batches(count, batch, rank, world):
            got = gather_known(rows, b)
            assert got.dim() == 1 and got.is_contiguous() and torch.equal(got.view(len(b), 8), rows[b])
            shared = gather_known(one, b)
            assert shared.shape == (8,) and torch.equal(shared, one[0])                    # K = 1: the one row, whatever the batch
            seen += b
    assert sorted(seen) == list(range(count))


# ------------------------------------------------------------------------------ 3. levels and columns
def test_schedule_of_a_5_step_matrix(repo_root):
    _, _, node = load_coeff_npz(repo_root / "weights/step_5_weight_00.npz")
    assert node.shape[0] == 6
    mean, data = known_schedule(node, "mean"), known_schedule(node, "data")
    assert len(mean) == len(data) == 6 and KNOWN_COLUMN0 == 2 ** 31
    for j in range(5):                                                                     # entry 0: the first input; entry k + 1: step k
        want = (float(np.float32(node[j, 1])), float(np.float32(node[j, 2])), 2 ** 31 + j)
        assert mean[j] == want and data[j] == want
        assert want[1] > 0.0
    assert mean[5] == (float(np.float32(node[5, 1])), 0.0, 2 ** 31 + 5)                    # the last step draws nothing
    assert data[5] == (1.0, 0.0, 2 ** 31 + 5)
    assert len({lv[2] for lv in mean}) == 6 and min(lv[2] for lv in mean) > node.shape[0]  # no collision with a matrix's columns (<= N + 1)
    with pytest.raises(ValueError):
        known_schedule(node, "sample")


# ------------------------------------------------------------------------------ 4. refusals, all before a GPU call
def test_check_known_refusals():
    E = 4 * EPI
    known, mask = torch.zeros(E), torch.zeros(E, dtype=torch.uint8)
    ok = dict(seed=1, fast_f32=False)
    assert check_known(known, mask, E, EPI, **ok) == (EPI, EPI)
    assert check_known(known[:EPI], mask, E, EPI, **ok) == (0, EPI)
    assert check_known(known, mask[:EPI], E, EPI, **ok) == (EPI, 0)
    assert check_known(known[:EPI], mask[:EPI], EPI, EPI, **ok) == (0, 0)
    for bad in (dict(known=None), dict(mask=None), dict(seed=None), dict(fast_f32=True), dict(epi=None), dict(epi=6), dict(epi=5 * EPI),
                dict(known=known[:2 * EPI]), dict(mask=mask[:EPI + 4]), dict(known=known.double()), dict(mask=mask.float()),
                dict(mask=mask != 0), dict(known=known.view(4, EPI)), dict(known=known[::2]), dict(mask=torch.zeros(E + 4, dtype=torch.uint8))):
        a = dict(known=known, mask=mask, epi=EPI, seed=1, fast_f32=False)
        a.update(bad)
        with pytest.raises(ValueError):
            check_known(a["known"], a["mask"], E, a["epi"], seed=a["seed"], fast_f32=a["fast_f32"])


def test_job_refusals_come_before_any_gpu_call(repo_root):
    """generate_sharded with a model that must never be called, on a device that need not exist: a bad argument is a ValueError from the host
    checks (anything later would fail differently)"""
    w = repo_root / "weights/step_5_weight_00.npz"
    u8 = torch.zeros((6, 32, 32, 3), dtype=torch.uint8)
    m = torch.ones((6, 32, 32), dtype=torch.bool)

    def never(*a):
        raise AssertionError("the denoiser was called")
    for known, mask, kf in ((u8, None, "mean"), (None, m, "mean"), (u8[:5], m, "mean"), (u8, m[:2], "mean"), (u8, m, "sample"),
                            (u8.float(), m, "mean"), (u8.permute(0, 3, 1, 2), m, "mean"), (u8, m.float(), "mean"),
                            (u8, torch.ones((6, 32, 32, 3), dtype=torch.bool), "mean"), (torch.zeros((6, 3, 32, 32), dtype=torch.float64), m, "mean")):
        with pytest.raises(ValueError):
            generate_sharded(never, w, 6, 4, known=known, mask=mask, known_final=kf)
