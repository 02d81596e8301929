"""The ideal denoiser on the GPU (include/natinf_ideal.h; naturaldiffusion_amd/ideal.py) against the fp64 numpy restatement of its definition
(tests/ideal_oracle.py): the staged weights, the posterior mean on exact-integer distances, its limits and ties, the same bytes for any split of the rows,
general floats under the softmax perturbation bound, and the denoiser as a sampling job's ``model_fn``.

Shapes (B, N, d): (5, 200, 64) one partial row block, a column tail, Np > N; (70, 333, 192) two row blocks, three column tiles with a tail;
(3, 130, 3072) CIFAR width; (CHUNK_ROWS + 44, 200, 64) crosses a row chunk; (5, K_RANGE + 70, 64) crosses a K range.

Integer-valued rows in 0..255 make every d2 an exact integer (tests/test_gpu_neighbours.py), so the logits are the oracle's bytes and what is left is the
weighted sum's own error, bounded by 2^-18 max|f|: at most 24 roundings of the fp32 accumulator plus a 16-term inner sum per 64 values of j, 2^-24 each, is
below 2^-18.6 of sum_j w_ij |f_j| <= max|f|; the weights' rounding and the final fp32 rounding add 2^-24 each."""
import numpy as np
import pytest
import torch

import ideal_oracle as O
from naturaldiffusion_amd import ideal as I

pytestmark = pytest.mark.gpu

SHAPES = [(5, 200, 64), (70, 333, 192), (3, 130, 3072), (I.CHUNK_ROWS + 44, 200, 64), (5, I.K_RANGE + 70, 64)]
IDS = ["5x200x64", "70x333x192", "3x130x3072", "chunk+44x200x64", "5xrange+70x64"]
X0_BOUND = 2.0 ** -18

_cache = {}


@pytest.fixture(scope="module")
def dev():
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _same_bytes(a, b):
    a, b = torch.as_tensor(a).cpu().contiguous(), torch.as_tensor(b).cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


def _np(t):
    return t.cpu().numpy()


def _int_case(shape, dev):
    """Integer-valued rows, c_i = 3 / std_j(d2_ij) (the largest weight between a few 1 / N and 0.99 on the oracle); everything the tests of a shape share:
    the device's outputs, its own distance table and weights, and the oracle on the exact distances -- computed once, never modified"""
    if shape not in _cache:
        B, N, d = shape
        rng = np.random.default_rng(100 + d + N)
        f = rng.integers(0, 256, (N, d)).astype(np.float32)
        u = rng.integers(0, 256, (B, d)).astype(np.float32)
        d2 = O.dist2(u, f)
        c = 3.0 / d2.std(1)
        alpha, sigma = np.linspace(0.9, 0.2, B), np.linspace(0.3, 0.95, B)
        x = (u * alpha[:, None]).astype(np.float32)
        train = I.TrainingSet(torch.from_numpy(f), device=dev)
        x0, out, st = I.posterior_mean(torch.from_numpy(u), c, train, x=torch.from_numpy(x), alpha=alpha, sigma=sigma, return_stats=True)
        ref = O.posterior_mean(u, c, f, d2=d2, x=x, alpha=alpha, sigma=sigma)
        _cache[shape] = dict(f=f, u=u, c=c, x=x, alpha=alpha, sigma=sigma, train=train, d2=d2, ref=ref, x0=x0, out=out, st=st)
    return _cache[shape]


# ---- 1. the weights ----

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_weights_are_the_softmax_of_the_devices_own_distances(dev, shape):
    from naturaldiffusion_amd import prdc as P
    k = _int_case(shape, dev)
    B, N, d = shape
    w, planes = I.debug_weights(torch.from_numpy(k["u"]), k["c"], k["train"])
    d2_dev = _np(P.debug_dist2(P.FeatureSet(torch.from_numpy(k["u"]), device=dev), k["train"].set))
    assert np.array_equal(d2_dev, k["d2"])                              # integer data: the exact table
    p = O.softmax_stats(d2_dev, k["c"])["p"]
    w = _np(w).astype(np.float64)
    err = np.abs(w - p.astype(np.float32).astype(np.float64))
    print(f"weights {shape}: max err / p = {np.max(err / np.maximum(p, 1e-300)):.3e}, row sums - 1 = {np.abs(w.sum(1) - 1).max():.3e}")
    assert (err <= 2.0 ** -23 * p + 2.0 ** -149).all()                  # one fp32 rounding and a double rounding; catches a dropped lo plane (2^-18)
    assert (np.abs(w.sum(1) - 1.0) <= N * 2.0 ** -24).all()
    planes = planes.float().cpu().numpy()
    assert planes.shape == (3, B, I.padded_cols(N)) and I.padded_cols(N) > N
    assert not planes[:, :, N:].any()                                   # pad columns
    assert np.array_equal((planes[0] + planes[1]) + planes[2], np.pad(w.astype(np.float32), ((0, 0), (0, I.padded_cols(N) - N))))
    assert planes[2].any() and planes[1].any()                          # the split really has three terms


# ---- 2. exact distances end to end ----

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_distance_posterior_mean(dev, shape):
    from naturaldiffusion_amd import neighbours as N_
    from naturaldiffusion_amd import prdc as P
    k = _int_case(shape, dev)
    ref, st = k["ref"], k["st"]
    assert k["x0"].dtype == torch.float32 and tuple(k["x0"].shape) == (shape[0], shape[2]) and k["x0"].is_cuda
    assert 2.0 / shape[1] < ref["pmax"].min() and ref["pmax"].max() < 0.999
    err = np.abs(_np(k["x0"]).astype(np.float64) - ref["x0"]).max()
    e_lse = np.abs(_np(st["lse"]) - ref["lse"]) / np.maximum(1.0, np.abs(ref["lse"]))
    e_pmax = np.abs(_np(st["pmax"]) - ref["pmax"])
    print(f"x0 {shape}: max err = 2^{np.log2(max(err, 1e-300) / 255.0):.2f} max|f|; lse {e_lse.max():.2e}; pmax {e_pmax.max():.2e}")
    assert err <= X0_BOUND * np.abs(k["f"]).max()
    assert (e_lse <= 1e-12).all() and (e_pmax <= 1e-12).all()
    assert st["nearest"].dtype == torch.int64 and np.array_equal(_np(st["nearest"]), ref["nearest"])
    _, idx = N_.nearest(P.FeatureSet(torch.from_numpy(k["u"]), device=dev), k["train"].set, k=1)
    assert torch.equal(st["nearest"], idx[:, 0])
    # the eps form: fp64 arithmetic on the unrounded mean, rounded once.  The mean's error (bounded above) enters scaled by alpha / sigma.
    tol = (k["alpha"] / k["sigma"])[:, None] * X0_BOUND * 255.0 + 2.0 ** -24 * np.abs(ref["out"])
    assert (np.abs(_np(k["out"]).astype(np.float64) - ref["out"]) <= tol).all()


# ---- 3. limits and ties ----

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_c_zero_is_the_column_mean_and_huge_c_the_nearest_row(dev, shape):
    k = _int_case(shape, dev)
    B, N, d = shape
    u = torch.from_numpy(k["u"])
    x0, st = I.posterior_mean(u, 0.0, k["train"], return_stats=True)
    mean = k["f"].astype(np.float64).mean(0)
    assert np.abs(_np(x0).astype(np.float64) - mean[None]).max() <= X0_BOUND * 255.0
    assert (np.abs(_np(st["pmax"]) - 1.0 / N) <= 1e-12).all() and (np.abs(_np(st["lse"]) - np.log(N)) <= 1e-12).all()
    assert np.array_equal(_np(st["nearest"]), k["ref"]["nearest"])      # chosen on d2: c = 0 makes every logit equal
    two = np.sort(k["d2"], 1)[:, :2]
    assert (two[:, 1] - two[:, 0] >= 1).all()                           # integer distances, no tie for the nearest row
    x0, st = I.posterior_mean(u, 1e6, k["train"], return_stats=True)
    assert np.array_equal(_np(x0), k["f"][k["ref"]["nearest"]]) and (_np(st["pmax"]) == 1.0).all()
    assert np.array_equal(_np(st["nearest"]), k["ref"]["nearest"])


def test_duplicate_training_rows_give_the_lower_index_and_that_row(dev):
    rng = np.random.default_rng(7)
    f = rng.integers(0, 256, (300, 192)).astype(np.float32)
    f[290] = f[17]                                                      # the two copies in the first and the third column tile
    f[131] = f[130]                                                     # ... and next to each other
    u = np.stack([f[17], f[130], f[17]]).copy()
    u[2, :5] += 1.0                                                     # near the copies, not on them
    train = I.TrainingSet(torch.from_numpy(f), device=dev)
    for c in (1e6, 1.0):                                                # every other row is further by > 10^5: its weight is exactly 0 at either scale
        x0, st = I.posterior_mean(torch.from_numpy(u), c, train, return_stats=True)
        assert _np(st["nearest"]).tolist() == [17, 130, 17], c
        assert np.array_equal(_np(x0), f[[17, 130, 17]]), c             # fp32(p) = 1/2 twice: 1/2 f + 1/2 f is exact
        assert np.allclose(_np(st["pmax"]), 0.5, rtol=1e-7, atol=0), c


def test_a_set_against_itself_leaves_the_own_row_out(dev):
    from naturaldiffusion_amd import neighbours as N_
    k = _int_case(SHAPES[1], dev)
    B, f, train = 70, k["f"], k["train"]
    s = 200                                                             # rows [200, 270) of the set: the left-out column is 200 + i
    rows = torch.from_numpy(f[s:s + B])
    d2 = O.dist2(f[s:s + B], f, self_offset=s)
    c = 3.0 / np.where(np.isinf(d2), np.nan, d2).std(1, where=~np.isinf(d2))
    ref = O.posterior_mean(f[s:s + B], c, f, d2=d2)
    x0, st = I.posterior_mean(rows, c, train, self_offset=s, return_stats=True)
    w, _ = I.debug_weights(rows, c, train, self_offset=s)
    own = np.arange(B), s + np.arange(B)
    assert (_np(w)[own] == 0.0).all() and not (_np(st["nearest"]) == own[1]).any()
    assert np.array_equal(_np(st["nearest"]), ref["nearest"])
    assert np.abs(_np(x0).astype(np.float64) - ref["x0"]).max() <= X0_BOUND * 255.0
    assert (np.abs(_np(st["lse"]) - ref["lse"]) <= 1e-12 * np.maximum(1, np.abs(ref["lse"]))).all()
    _, idx = N_.nearest(train.set, train.set, k=1, row_range=range(s, s + B), self_offset=0)
    assert torch.equal(st["nearest"], idx[:, 0])
    x0, st = I.posterior_mean(rows, 1e6, train, self_offset=s, return_stats=True)      # without the select the own row (d2 = 0) would take everything
    assert np.array_equal(_np(x0), f[ref["nearest"]]) and (_np(st["pmax"]) == 1.0).all()
    x0, st = I.posterior_mean(rows, 0.0, train, self_offset=s, return_stats=True)      # 0 * inf: the left-out row stays out of the plain mean too
    want = (f.astype(np.float64).sum(0)[None] - f[s:s + B]) / (len(f) - 1)
    assert np.abs(_np(x0).astype(np.float64) - want).max() <= X0_BOUND * 255.0 and (np.abs(_np(st["pmax"]) - 1 / (len(f) - 1)) <= 1e-12).all()


def test_a_scale_outside_the_contract_stays_in_its_row(dev):
    """include/natinf_ideal.h: the values of a device-side c are not inspected; a NaN makes its own row NaN (nearest is chosen on d2) and no other"""
    k = _int_case(SHAPES[1], dev)
    c = torch.from_numpy(k["c"]).to(dev)
    c[3] = float("nan")
    x0, out, st = I.posterior_mean(torch.from_numpy(k["u"]), c, k["train"], x=torch.from_numpy(k["x"]), alpha=k["alpha"], sigma=k["sigma"], return_stats=True)
    keep = torch.arange(70, device=dev) != 3
    assert torch.isnan(x0[3]).all() and torch.isnan(out[3]).all() and torch.isnan(st["lse"][3]) and torch.isnan(st["pmax"][3])
    assert _same_bytes(x0[keep], k["x0"][keep]) and _same_bytes(out[keep], k["out"][keep]) and _same_bytes(st["lse"][keep], k["st"]["lse"][keep])
    assert torch.equal(st["nearest"], k["st"]["nearest"])


# ---- 4. a row function ----

def _call(k, sel):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel]))
    x0, out, st = I.posterior_mean(t(k["u"]), k["c"][sel], k["train"], x=t(k["x"]), alpha=k["alpha"][sel], sigma=k["sigma"][sel], return_stats=True)
    return dict(x0=x0, out=out, lse=st["lse"], pmax=st["pmax"], nearest=st["nearest"])


def _whole(k):
    return dict(x0=k["x0"], out=k["out"], lse=k["st"]["lse"], pmax=k["st"]["pmax"], nearest=k["st"]["nearest"])


def test_any_split_or_order_of_the_rows_gives_the_same_bytes(dev):
    k = _int_case(SHAPES[1], dev)
    whole = _whole(k)
    parts = [_call(k, np.arange(a, b)) for a, b in ((0, 1), (1, 64), (64, 70))]
    perm = np.random.default_rng(3).permutation(70)
    shuffled = _call(k, perm)
    for key, v in whole.items():
        assert _same_bytes(torch.cat([p[key] for p in parts]), v), key
        assert _same_bytes(shuffled[key], v[torch.from_numpy(perm).to(v.device)]), key


def test_a_chunk_crossing_call_equals_its_rows_called_alone(dev):
    k = _int_case(SHAPES[3], dev)
    whole = _whole(k)
    B = SHAPES[3][0]
    for sel in (np.array([0]), np.array([I.CHUNK_ROWS - 1]), np.array([I.CHUNK_ROWS]), np.arange(I.CHUNK_ROWS - 3, I.CHUNK_ROWS + 5), np.array([B - 1])):
        alone = _call(k, sel)
        for key, v in whole.items():
            assert _same_bytes(alone[key], v[torch.from_numpy(sel).to(v.device)]), (key, sel)


# ---- 5. general floats ----

def test_general_floats_within_the_softmax_perturbation_bound(dev):
    """Logits within eta of the exact ones change the weights' l1 norm by at most e^(2 eta) - 1: |x0 - ref| <= max|f| (expm1(2 c delta_i) + 2^-18) with
    delta_i the measured error of the device's own distances"""
    from naturaldiffusion_amd import prdc as P
    rng = np.random.default_rng(11)
    f, u = rng.standard_normal((333, 192)).astype(np.float32), rng.standard_normal((70, 192)).astype(np.float32)
    c = 0.5
    train = I.TrainingSet(torch.from_numpy(f), device=dev)
    x0, st = I.posterior_mean(torch.from_numpy(u), c, train, return_stats=True)
    ref = O.posterior_mean(u, c, f)
    d2_dev = _np(P.debug_dist2(P.FeatureSet(torch.from_numpy(u), device=dev), train.set))
    delta = np.abs(d2_dev - O.dist2(u, f)).max(1)
    err = np.abs(_np(x0).astype(np.float64) - ref["x0"]).max(1)
    bound = np.abs(f).max() * (np.expm1(2 * c * delta) + X0_BOUND)
    print(f"floats: delta max {delta.max():.3e}, err max {err.max():.3e}, tightest bound {bound.min():.3e}")
    assert (err <= bound).all()
    assert np.array_equal(_np(st["nearest"]), np.argmin(d2_dev, 1))


# ---- 6. as a model_fn ----

def _job(dev):
    if "job" not in _cache:
        from naturaldiffusion_amd import CIFAR10NaturalInference as M
        from naturaldiffusion_amd import coeffgen
        train_u8 = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (130, 32, 32, 3), dtype=np.uint8))
        den = M.ideal_denoiser(train_u8, dev)
        coeff = coeffgen.ddim_vp_continuous(coeffgen.quadratic_time_grid(10))
        imgs, idx = M.generate_sharded(den, None, 6, 6, device=dev, coeff=coeff)
        _cache["job"] = (train_u8, den, coeff, imgs, idx)
    return _cache["job"]


def test_a_sampling_job_with_the_ideal_denoiser_copies_the_training_set(dev):
    from naturaldiffusion_amd import CIFAR10NaturalInference as M
    train_u8, den, coeff, imgs, idx = _job(dev)
    assert imgs.dtype == torch.uint8 and tuple(imgs.shape) == (6, 32, 32, 3) and idx.tolist() == list(range(6))
    res = M.calc_nearest(imgs, train_u8, dev, space="pixel", k=2)
    print("nearest / second nearest:", res["d2"][:, 0], res["d2"][:, 1])
    assert (res["d2"][:, 0] <= 1e-2 * res["d2"][:, 1]).all()            # a sampler that does not copy sits at a ratio near 1


def test_two_ranks_generate_one_ranks_bytes(dev):
    from naturaldiffusion_amd import CIFAR10NaturalInference as M
    train_u8, den, coeff, imgs, idx = _job(dev)
    merged = torch.empty_like(imgs)
    for rank in (0, 1):
        part, pidx = M.generate_sharded(den, None, 6, 2, rank=rank, world=2, device=dev, coeff=coeff)
        assert pidx.tolist() == list(range(rank, 6, 2))
        merged[pidx] = part
    assert torch.equal(merged, imgs)


def test_denoiser_gap_of_the_ideal_denoiser_against_itself(dev):
    from naturaldiffusion_amd import CIFAR10NaturalInference as M
    train_u8, den, coeff, imgs, idx = _job(dev)
    ts = [1.0, 0.4, 1e-3]
    res = M.calc_denoiser_gap(den, den, ts, rows=[0, 3, 64, 129], seed=5)
    assert all(res[key].shape == (3,) and res[key].dtype == np.float64 for key in ("t", "gap", "ideal_mse", "pmax", "own"))
    assert (res["gap"] == 0.0).all() and res["own"][-1] == 1.0
    assert res["ideal_mse"][-1] < 1e-4 < res["ideal_mse"][0] and (res["pmax"] > 1 / 130).all() and res["pmax"][-1] > 0.999
    other = lambda x, labels: den(x, labels) + 0.25                     # a denoiser that is off by a constant: gap = (sigma / alpha)^2 / 16
    off = M.calc_denoiser_gap(other, den.train, ts, rows=[0, 3, 64, 129], seed=5)
    alpha, sigma = I.levels_of_labels(np.array([np.float32(t) * np.float32(999) for t in ts]))
    assert np.allclose(off["gap"], (sigma / alpha) ** 2 / 16, rtol=1e-5) and np.array_equal(off["pmax"], res["pmax"])
