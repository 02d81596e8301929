"""Host pieces of CIFAR10 colorization (no GPU): the basis and its inverse, the fp32 blend replayed in numpy against its fp64 evaluation, the level
and column schedule, the gray-channel preparation of the job, and the refusals, which all come before any GPU call."""
import numpy as np
import pytest
import torch

from naturaldiffusion_amd.CIFAR10NaturalInference import gather_known, generate_sharded, prepare_gray, u8_to_centered
from naturaldiffusion_amd.coeff import load_coeff_npz
from naturaldiffusion_amd.sampler import (COLOR_COLUMN0, COLOR_M, COLOR_W, KNOWN_COLUMN0, check_gray, color_blend_host, color_schedule,
                                          decouple0_host, known_schedule)

EPI = 3 * 32 * 32
ULP = 2.0 ** -24


# ------------------------------------------------------------------------------ 1. the basis
def test_inverse_is_the_correctly_rounded_fp64_inverse():
    assert COLOR_M.dtype == np.float32 and COLOR_W.dtype == np.float32 and COLOR_M.shape == COLOR_W.shape == (3, 3)
    M64 = COLOR_M.astype(np.float64)
    assert np.array_equal(COLOR_W, np.linalg.inv(M64).astype(np.float32))
    res = np.abs(M64 @ COLOR_W.astype(np.float64) - np.eye(3)).max()
    print("max |M W - I| =", res)
    assert res <= 2.6e-8 * 1.01
    assert np.abs(M64.T @ M64 - np.eye(3)).max() < 1e-6                                    # orthonormal, to fp32
    assert np.abs(M64[:, 0] - 1 / np.sqrt(3)).max() < 1e-6                                 # column 0 is the gray direction


# ------------------------------------------------------------------------------ 2. the arithmetic
@pytest.mark.parametrize("scale", [1.0, 4.0])
def test_blend_against_fp64(scale):
    """400,000 random pixels.  Bound 16 * 2^-24 * s, s = max(1, |target u0|, max |M^T x|): each dot3 is three roundings, the absolute row sums
    of M and W are at most 1.74, the W M - I residual is about half an ulp: about 13 ulp * s together."""
    n = 400000
    rs = np.random.RandomState(int(scale))
    x = (rs.randn(n, 3, 1) * scale).astype(np.float32)
    g = (rs.randn(n, 1) * scale).astype(np.float32)
    z = rs.randn(n, 1).astype(np.float32)
    alpha, std = 0.8, 0.6
    out = color_blend_host(x, g, alpha, std, z)
    assert out.dtype == np.float32 and out.shape == x.shape
    M64 = COLOR_M.astype(np.float64)
    target = g.astype(np.float64) * np.float64(np.float32(alpha)) + z.astype(np.float64) * np.float64(np.float32(std))
    lat_in = np.einsum("nip,ij->njp", x.astype(np.float64), M64)
    lat_out = np.einsum("nip,ij->njp", out.astype(np.float64), M64)
    s = np.maximum(1.0, np.maximum(np.abs(target), np.abs(lat_in).max(axis=1)))
    bound = 16 * ULP * s
    e_gray = np.abs(lat_out[:, 0] - target)
    e_rest = np.abs(lat_out[:, 1:] - lat_in[:, 1:])
    lat = lat_in.copy()
    lat[:, 0] = target
    ref = np.einsum("nip,ij->njp", lat, np.linalg.inv(M64))                                # the reference formula (:142, mask (1, 0, 0)) in fp64
    e_img = np.abs(out.astype(np.float64) - ref)
    print(f"scale {scale}: gray {np.max(e_gray / s) / ULP:.2f}, rest {np.max(e_rest / s[:, None]) / ULP:.2f}, image {np.max(e_img / s[:, None]) / ULP:.2f} ulp*s")
    assert (e_gray <= bound).all()
    assert (e_rest <= bound[:, None]).all()
    assert (e_img <= bound[:, None]).all()


def test_blend_without_a_draw_and_the_gray_channel_of_a_picture():
    rs = np.random.RandomState(3)
    x = rs.randn(5, 3, 64).astype(np.float32)
    g = rs.randn(5, 64).astype(np.float32)
    a = color_blend_host(x, g, 0.9993, 0.0)                                                # z0 is not read
    b = color_blend_host(x, g, 0.9993, 0.0, np.full((5, 64), np.nan, np.float32))
    assert np.array_equal(a, b) and np.isfinite(a).all()
    assert np.array_equal(color_blend_host(x, g[:1], 0.5, 0.25, g), color_blend_host(x, np.repeat(g[:1], 5, 0), 0.5, 0.25, g))   # one shared picture
    k = rs.randn(2, 3, 32, 32).astype(np.float32)
    u = decouple0_host(k)
    assert u.dtype == np.float32 and u.shape == (2, 32, 32)
    M = COLOR_M
    assert np.array_equal(u, (k[:, 0] * M[0, 0] + k[:, 1] * M[1, 0]) + k[:, 2] * M[2, 0])
    S = np.einsum("nihw,i->nhw", np.abs(k).astype(np.float64), np.abs(M[:, 0]).astype(np.float64))
    assert (np.abs(u - np.einsum("nihw,i->nhw", k.astype(np.float64), M[:, 0].astype(np.float64))) <= 5 * ULP * S).all()      # five roundings, each of a value <= S
    # a NaN of x reaches all three outputs of its pixel, and only that pixel
    x[0, 1, 7] = np.nan
    o = color_blend_host(x, g, 0.5, 0.0)
    assert np.isnan(o[0, :, 7]).all() and np.isnan(o).sum() == 3
    with pytest.raises(ValueError):
        decouple0_host(np.zeros((4, 32, 32), np.float32))


# ------------------------------------------------------------------------------ 3. levels and columns
def test_schedule_of_a_5_step_matrix(repo_root):
    _, _, node = load_coeff_npz(repo_root / "weights/step_5_weight_00.npz")
    assert node.shape[0] == 6 and COLOR_COLUMN0 == 2 ** 31 + 2 ** 30 == 0xC0000000
    mean, data = color_schedule(node, "mean"), color_schedule(node, "data")
    assert len(mean) == len(data) == 6
    for j in range(5):                                                                     # entry 0: the first input; entry k + 1: step k
        want = (float(np.float32(node[j, 1])), float(np.float32(node[j, 2])), COLOR_COLUMN0 + j)
        assert mean[j] == want and data[j] == want and want[1] > 0.0
    assert mean[5] == (float(np.float32(node[5, 1])), 0.0, COLOR_COLUMN0 + 5)              # the last step draws nothing
    assert data[5] == (1.0, 0.0, COLOR_COLUMN0 + 5)
    for mode in ("mean", "data"):                                                          # known_schedule's levels, other columns
        ks, cs = known_schedule(node, mode), color_schedule(node, mode)
        assert [lv[:2] for lv in ks] == [lv[:2] for lv in cs]
        assert not {lv[2] for lv in ks} & {lv[2] for lv in cs}
    assert min(lv[2] for lv in mean) > KNOWN_COLUMN0 + node.shape[0] and max(lv[2] for lv in mean) < 2 ** 32
    with pytest.raises(ValueError):
        color_schedule(node, "sample")


# ------------------------------------------------------------------------------ 4. the job's gray pictures
def test_prepare_gray_formats():
    rs = np.random.RandomState(0)
    g8 = torch.from_numpy(rs.randint(0, 256, size=(5, 32, 32)).astype(np.uint8))
    a = prepare_gray(g8, 5)
    assert a.shape == (5, 1024) and a.dtype == torch.float32 and a.is_contiguous() and a.device.type == "cpu"
    ggg = g8[..., None].expand(-1, -1, -1, 3).contiguous()
    assert torch.equal(prepare_gray(ggg, 5), a)                                            # a gray picture == its (g, g, g) expansion
    c = u8_to_centered(g8).numpy()
    assert np.array_equal(a.numpy().reshape(5, 32, 32), decouple0_host(np.stack([c, c, c], axis=1)))
    u8 = torch.from_numpy(rs.randint(0, 256, size=(5, 32, 32, 3)).astype(np.uint8))
    f32 = u8_to_centered(u8.permute(0, 3, 1, 2)).contiguous()
    b = prepare_gray(u8, 5)
    assert torch.equal(b, prepare_gray(f32, 5)) and not torch.equal(a, b)
    assert np.array_equal(b.numpy().reshape(5, 32, 32), decouple0_host(f32.numpy()))       # of a colour picture, its gray channel
    one = prepare_gray(g8[:1], 5)                                                          # K = 1
    assert one.shape == (1, 1024) and torch.equal(one[0], a[0])
    assert torch.equal(gather_known(one, [3, 4]), a[0]) and torch.equal(gather_known(a, [3, 1]), a[[3, 1]].reshape(-1))


def test_prepare_gray_refusals():
    g8 = torch.zeros((6, 32, 32), dtype=torch.uint8)
    for bad in (g8[:5], g8[:2], g8.float(), g8[:, :16], torch.zeros((6, 3, 32, 32), dtype=torch.uint8), torch.zeros((6, 32, 32, 3)),
                torch.zeros((6, 3, 32, 32), dtype=torch.float64), torch.zeros((6, 1, 32, 32)), torch.zeros((6, 32, 32, 1), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            prepare_gray(bad, 6)
    with pytest.raises(ValueError):
        prepare_gray(g8, 6, "sample")


def test_check_gray_refusals():
    E = 4 * EPI
    g = torch.zeros(E // 3)
    ok = dict(seed=1, fast_f32=False)
    assert check_gray(g, E, EPI, **ok) == EPI // 3
    assert check_gray(g[:EPI // 3], E, EPI, **ok) == 0
    assert check_gray(g[:EPI // 3], EPI, EPI, **ok) == 0
    assert check_gray(torch.zeros(5 * 8), 5 * 24, 24, **ok) == 8
    for bad in (dict(g=None), dict(seed=None), dict(fast_f32=True), dict(epi=None), dict(epi=6), dict(epi=5 * EPI), dict(epi=16, E=64),
                dict(g=g[:2 * EPI // 3]), dict(g=torch.zeros(E)), dict(g=g.double()), dict(g=g.view(4, -1)), dict(g=torch.zeros(2 * E // 3)[::2])):
        a = dict(g=g, epi=EPI, E=E, seed=1, fast_f32=False)
        a.update(bad)
        with pytest.raises(ValueError):
            check_gray(a["g"], a["E"], a["epi"], seed=a["seed"], fast_f32=a["fast_f32"])


def test_job_refusals_come_before_any_gpu_call(repo_root):
    """generate_sharded with a model that must never be called, on a device that need not exist: a bad argument is a ValueError from the host
    checks (anything later would fail differently)"""
    w = repo_root / "weights/step_5_weight_00.npz"
    g8 = torch.zeros((6, 32, 32), dtype=torch.uint8)
    u8 = torch.zeros((6, 32, 32, 3), dtype=torch.uint8)
    m = torch.ones((6, 32, 32), dtype=torch.bool)

    def never(*a):
        raise AssertionError("the denoiser was called")
    for kw in (dict(gray=g8, known=u8, mask=m), dict(gray=g8, known=u8), dict(gray=g8, mask=m), dict(gray=g8[:5]), dict(gray=g8.float()),
               dict(gray=g8, known_final="sample"), dict(gray=torch.zeros((6, 3, 32, 32), dtype=torch.uint8))):
        with pytest.raises(ValueError):
            generate_sharded(never, w, 6, 4, **kw)
