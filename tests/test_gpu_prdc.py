"""k-nearest-neighbour manifold metrics on the GPU (include/natinf_prdc.h; naturaldiffusion_amd/prdc.py) against tests/prdc_oracle.py: the planes bit for
bit, the distance tiles within BAND of fp64 and no further from it than torch's fp32 statement, radii and counts inside what BAND allows, the same bytes
for any split of the rows, the four numbers, offsets past 2^31 and the public path.

BAND bounds |d2_gpu - d2_fp64| / (|a|^2 + |b|^2): twice the largest value measured on the MI355X at the two shapes of test_distance_band, rounded up to a
power of two (DESIGN.md section 4d-prdc has the figures).  The cluster inputs were verified in fp64 for BAND <= 2^-16 only, hence the condition below."""
import numpy as np
import pytest
import torch

import prdc_oracle as O

pytestmark = pytest.mark.gpu

BAND = 2.0 ** -21
assert BAND <= 2.0 ** -16

_cache = {}


@pytest.fixture(scope="module")
def dev():
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _pair(n_real, n_gen, d):
    """(real, gen) cluster features on the host, the fp64 distances gen x real and both sets' own distance matrices: computed once, never modified"""
    key = (n_real, n_gen, d)
    if key not in _cache:
        real, gen = O.cluster_feats(n_real, d, 0.0, 1), O.cluster_feats(n_gen, d, 0.6, 2)
        _cache[key] = dict(real=real, gen=gen, d2=O.dist2(gen, real), scale=O.norm_sums(gen, real),
                           d2_real=O.dist2(real, real), d2_gen=O.dist2(gen, gen))
    return _cache[key]


def _fs(x, dev):
    from naturaldiffusion_amd import prdc as P
    return P.FeatureSet(x, device=dev)


def _sq(x):
    return (x.double() ** 2).sum(1)


def test_planes_and_norms(dev):
    for n, d in ((1, 64), (257, 192), (70, 4096)):
        x = O.cluster_feats(n, d, 0.3, 5) - 0.2                  # both signs, many zeros' neighbours
        x[0, :4] = torch.tensor([1.0, -3.0e-5, 65504.0, 1.0 + 2.0 ** -23])
        fs = _fs(x, dev)
        pl = fs.planes.float().cpu()
        assert fs.planes.dtype == torch.bfloat16 and tuple(fs.planes.shape) == (3, n, d)
        assert torch.equal((pl[0] + pl[1]) + pl[2], x), (n, d)
        ref = _sq(x)
        assert float(((fs.norms.cpu() - ref).abs() / ref).max()) <= 1e-14, (n, d)


@pytest.mark.parametrize("n_rows,n_cols,d", [(130, 257, 192), (300, 261, 2048)])
def test_distance_band(dev, n_rows, n_cols, d):
    """the tile arithmetic against fp64, beside torch's fp32 statement on the same device and inputs"""
    from naturaldiffusion_amd import prdc as P
    c = _pair(n_cols, n_rows, d)                                 # rows = gen, columns = real
    got = P.debug_dist2(_fs(c["gen"], dev), _fs(c["real"], dev)).cpu()
    a, b = c["gen"].to(dev), c["real"].to(dev)
    stmt = ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.t())).cpu().double()
    err = float(((got - c["d2"]).abs() / c["scale"]).max())
    err_torch = float(((stmt - c["d2"]).abs() / c["scale"]).max())
    print(f"prdc band ({n_rows}, {n_cols}, {d}): kernel {err:.3e} = 2^{np.log2(max(err, 1e-300)):.2f}, torch fp32 {err_torch:.3e} = 2^{np.log2(err_torch):.2f}")
    assert (got >= 0).all()
    assert err <= err_torch, (err, err_torch)
    assert err <= BAND, (err, BAND)


def _radii_case(dev, n_rows, n_cols, d, k):
    from naturaldiffusion_amd import prdc as P
    c = _pair(n_cols, n_rows, d)
    got = P._knn(_fs(c["gen"], dev), range(n_rows), _fs(c["real"], dev), k, -1).cpu()
    ref = O.kth(c["d2"], k)
    bound = BAND * (_sq(c["gen"]) + _sq(c["real"]).max())
    assert (got >= 0).all() and ((got - ref).abs() <= bound).all(), float(((got - ref).abs() / bound).max())


@pytest.mark.parametrize("n_rows,n_cols,d,k", [(1, 2, 64, 1), (130, 257, 192, 3), (300, 261, 2048, 5), (130, 257, 192, 8), (1, 2, 64, 2)])
def test_radii(dev, n_rows, n_cols, d, k):
    """an order statistic moves by no more than its inputs"""
    _radii_case(dev, n_rows, n_cols, d, k)


def test_radii_of_a_set_against_itself(dev):
    from naturaldiffusion_amd import prdc as P
    c = _pair(257, 130, 192)
    x = c["real"]
    got = P.knn_radii(_fs(x, dev), 3).cpu()
    ref = O.kth(O.mask_self(c["d2_real"], 0), 3)
    assert ((got - ref).abs() <= BAND * (_sq(x) + _sq(x).max())).all()
    # without the exclusion every row's nearest column is itself
    zero = P._knn(_fs(x, dev), range(257), _fs(x, dev), 1, -1).cpu()
    assert (zero >= 0).all() and (zero <= BAND * 2 * _sq(x)).all()


def test_identical_rows_give_a_radius_inside_the_band_never_a_negative_one(dev):
    from naturaldiffusion_amd import prdc as P
    x = O.cluster_feats(50, 64, 0.0, 9).clone()
    x[7] = x[3]
    r2 = P.knn_radii(_fs(x, dev), 1).cpu()
    assert (r2 >= 0).all()
    for i in (3, 7):
        assert float(r2[i]) <= BAND * 2 * float(_sq(x)[i])
    ref = O.radii(x, 1)
    assert ((r2 - ref).abs() <= BAND * (_sq(x) + _sq(x).max())).all()


@pytest.mark.parametrize("n_rows,n_cols,d", [(130, 257, 192), (300, 261, 2048)])
def test_counts_lie_in_the_band_interval(dev, n_rows, n_cols, d):
    from naturaldiffusion_amd import prdc as P
    c = _pair(n_cols, n_rows, d)
    k = 3
    r2_rows, r2_cols = O.kth(O.mask_self(c["d2_gen"], 0), k), O.kth(O.mask_self(c["d2_real"], 0), k)         # exact radii in: the band is the distances' alone
    zero_r, zero_c = torch.zeros_like(r2_rows), torch.zeros_like(r2_cols)
    (lo_r, lo_c), (hi_r, hi_c) = O.count_interval(c["d2"], BAND * c["scale"], r2_rows, r2_cols, zero_r, zero_c)
    fragile = float(((lo_r != hi_r) | (lo_c != hi_c)).double().mean())
    assert fragile <= 0.02, f"{fragile:.3f} of the rows sit within the band of a radius: the interval would hide a wrong kernel"
    rows, cols = _fs(c["gen"], dev), _fs(c["real"], dev)
    cr, cc = P._balls(rows, range(n_rows), cols, r2_rows.to(dev), r2_cols.to(dev))
    assert cr.dtype == torch.int32 and cc.dtype == torch.int32
    cr, cc = cr.cpu().long(), cc.cpu().long()
    assert ((lo_r <= cr) & (cr <= hi_r)).all() and ((lo_c <= cc) & (cc <= hi_c)).all()
    assert 0.1 <= float((cc > 0).double().mean()) <= 0.99 and 0.1 <= float((cr > 0).double().mean()) <= 0.99, "the case decides nothing"
    only_r, none = P._balls(rows, range(n_rows), cols, r2_rows.to(dev), None)
    assert none is None and torch.equal(only_r.cpu().long(), cr)
    none, only_c = P._balls(rows, range(n_rows), cols, None, r2_cols.to(dev))
    assert none is None and torch.equal(only_c.cpu().long(), cc)


def test_a_row_slice_gives_the_bytes_of_the_whole_call(dev):
    from naturaldiffusion_amd import prdc as P
    c = _pair(257, 130, 192)
    a, g = _fs(c["real"], dev), _fs(c["gen"], dev)
    sl = range(64, 193)
    whole = P.knn_radii(a, 3)
    assert torch.equal(P.knn_radii(a, 3, sl), whole[64:193])
    r2_gen = P.knn_radii(g, 3)
    wr, wc = P._balls(a, range(257), g, whole, r2_gen)
    sr, sc = P._balls(a, sl, g, whole[64:193], r2_gen)
    assert torch.equal(sr, wr[64:193]) and torch.equal(sc, wc[64:193])
    # a set against itself, counted: the left-out column follows the slice
    wr, _ = P._balls(a, range(257), a, whole, None, self_offset=0)
    sr, _ = P._balls(a, sl, a, whole[64:193], None, self_offset=64)
    assert torch.equal(sr, wr[64:193]) and int(wr.min()) >= 3          # the k = 3 ball holds its three neighbours: d2_ij is the same bytes in both kernels
    one = P.prdc_counts(a, g, 3)
    for world in (2, 3):
        parts = [P.prdc_counts(a, g, 3, P.row_slice(257, r, world), P.row_slice(130, r, world), r2_real=one["r2_real"], r2_gen=one["r2_gen"])
                 for r in range(world)]                                # the whole sets' radii handed on: computed once
        for key in ("gen_in_real_balls", "real_in_gen_balls", "gen_in_own_ball"):
            assert torch.equal(torch.cat([p[key] for p in parts]), one[key]), (world, key)
        assert np.array_equal(sum(P.count_sums(p) for p in parts), P.count_sums(one))
    own = P.prdc_counts(a, g, 3, P.row_slice(257, 1, 3), P.row_slice(130, 1, 3))       # ... or computed by the call itself: the same bytes
    assert torch.equal(own["r2_real"], one["r2_real"]) and torch.equal(own["r2_gen"], one["r2_gen"])
    for key in ("gen_in_real_balls", "real_in_gen_balls", "gen_in_own_ball"):
        assert torch.equal(own[key], parts[1][key]), key
    with pytest.raises(ValueError, match="r2_real"):
        P.prdc_counts(a, g, 3, r2_real=one["r2_gen"])
    with pytest.raises(ValueError, match="feature width"):
        P._knn(a, range(257), _fs(O.cluster_feats(20, 64, 0.0, 1), dev), 3, -1)


def test_the_four_numbers_at_their_ends(dev):
    from naturaldiffusion_amd import prdc as P
    x = _pair(257, 130, 192)["real"]
    m = P.prdc(x.to(dev), x.to(dev), k=3)
    assert m["precision"] == 1.0 and m["recall"] == 1.0 and m["coverage"] == 1.0 and m["density"] >= 1.0
    far = _pair(257, 130, 192)["gen"].clone()
    far[:, 0] += 100.0 * float(_sq(x).max().sqrt())                     # a hundred norms away
    m = P.prdc(_fs(x, dev), _fs(far, dev), k=3)
    assert m == dict(precision=0.0, recall=0.0, density=0.0, coverage=0.0)


@pytest.mark.parametrize("n_real,n_gen,d,k", [(257, 130, 192, 3), (261, 300, 2048, 5), (130, 257, 64, 1)])
def test_the_four_numbers_against_fp64(dev, n_real, n_gen, d, k):
    """every count vector inside its fp64 interval (distances and radii both within the band), hence each number inside its own; equal to the fp64 number
    wherever no row is fragile"""
    from naturaldiffusion_amd import prdc as P
    c = _pair(n_real, n_gen, d)
    real, gen = c["real"], c["gen"]
    r2_real, r2_gen = O.kth(O.mask_self(c["d2_real"], 0), k), O.kth(O.mask_self(c["d2_gen"], 0), k)
    br_real, br_gen = BAND * (_sq(real) + _sq(real).max()), BAND * (_sq(gen) + _sq(gen).max())
    band = BAND * c["scale"]
    none_r, none_c = torch.zeros(n_gen, dtype=torch.float64), torch.zeros(n_real, dtype=torch.float64)
    (_, g_lo), (_, g_hi) = O.count_interval(c["d2"], band, none_r, r2_real, none_r, br_real)                 # rows gen, columns real
    (o_lo, r_lo), (o_hi, r_hi) = O.count_interval(c["d2"].t(), band.t(), r2_real, r2_gen, br_real, br_gen)   # rows real, columns gen
    fragile = [float((lo != hi).double().mean()) for lo, hi in ((g_lo, g_hi), (r_lo, r_hi), (o_lo, o_hi))]
    assert max(fragile) <= 0.02, fragile
    got = P.prdc(_fs(real, dev), _fs(gen, dev), k=k)
    ref = O.prdc(real, gen, k)
    mean = lambda v: float((v > 0).double().mean())
    ivals = dict(precision=(mean(g_lo), mean(g_hi)), recall=(mean(r_lo), mean(r_hi)), coverage=(mean(o_lo), mean(o_hi)),
                 density=(float(g_lo.double().mean()) / k, float(g_hi.double().mean()) / k))
    for name, (lo, hi) in ivals.items():
        assert lo - 1e-12 <= got[name] <= hi + 1e-12, (name, lo, got[name], hi)
        assert lo - 1e-12 <= ref[name] <= hi + 1e-12, (name, lo, ref[name], hi)
        if lo == hi:
            assert abs(got[name] - ref[name]) <= 1e-12, (name, got[name], ref[name])
        assert 0.05 <= ref[name] <= (3.0 if name == "density" else 0.99), (name, ref[name])


def test_offsets_past_two_to_the_31(dev):
    """524,800 x 2048 columns: the third plane starts 2.1e9 elements into the buffer, the last rows 1.07e9 elements into a plane"""
    from naturaldiffusion_amd import prdc as P
    n, d, k, s = 524800, 2048, 3, 524700
    g = torch.Generator(device=dev).manual_seed(3)
    W = torch.randn(6, d, generator=g, device=dev)
    x = torch.randn(n, d, generator=g, device=dev).mul_(0.3)
    x.addmm_(torch.randn(n, 6, generator=g, device=dev), W).relu_().mul_(0.5)
    fs = P.FeatureSet(x, device=dev)
    assert 2 * n * d > 2 ** 31
    got = P.knn_radii(fs, k, range(s, s + 96))
    rows = x[s:s + 96]
    ref = O.kth(O.mask_self(O.dist2(rows, x), s), k)
    bound = BAND * (_sq(rows) + float((fs.norms).max()))
    assert ((got - ref).abs() <= bound).all(), float(((got - ref).abs() / bound).max())
    assert (ref > 1e3 * bound).all(), "the radii are not resolved by the bound"


_RANK_SCRIPT = r"""
import os, sys, json
import torch, torch.distributed as dist
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
import prdc_oracle as O
from naturaldiffusion_amd import CIFAR10NaturalInference as M
from naturaldiffusion_amd import prdc as P
dev = torch.device("cuda:0")
real, gen = O.cluster_feats(257, 192, 0.0, 1), O.cluster_feats(130, 192, 0.6, 2)
one = P.prdc_from_sums(P.count_sums(P.prdc_counts(P.FeatureSet(real, device=dev), P.FeatureSet(gen, device=dev), 3)), 3)      # no collective
both = P.prdc(real.to(dev), gen.to(dev), k=3)                                 # row slices + the all-reduce


class Lookup:                                                                 # stands for the Inception engine: image i is the picture of feature row i
    max_batch = 50

    def __call__(self, imgs):
        return gen.to(dev)[imgs[:, 0, 0, 0].long().to(dev)]


imgs = torch.zeros(130, 2, 2, 3, dtype=torch.uint8)
imgs[:, 0, 0, 0] = torch.arange(130, dtype=torch.uint8)
mine = imgs[rank::world] if rank else imgs[rank::world][:-3]                  # ragged shares: 62 and 65 images, 127 in all
sharded = M.calc_prdc_sharded(mine, real.numpy(), dev, model=Lookup(), k=3)
with open({out!r} + f"/rank{{rank}}.json", "w") as fh:                          # (two ranks' lines on one stdout can run into each other)
    json.dump(dict(rank=rank, one=one, both=both, sharded=sharded, n_local=len(mine)), fh)
dist.destroy_process_group()
"""


def test_two_ranks_give_one_ranks_numbers(dev, tmp_path):
    """prdc() in a process group of two (gloo, both ranks on cuda:0) equals the single-process numbers; calc_prdc_sharded all-gathers ragged shares of
    features and equals prdc() on the gathered set, whatever order the gather leaves the rows in"""
    import json, os, subprocess, sys
    from pathlib import Path
    from naturaldiffusion_amd import prdc as P
    root = Path(__file__).resolve().parent.parent
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT.format(root=str(root), out=str(tmp_path)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    import socket
    with socket.socket() as s:                                        # a port that is free now: another copy of the suite on this host takes another
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = [json.loads((tmp_path / f"rank{r}.json").read_text()) for r in (0, 1)]
    assert [r["rank"] for r in res] == [0, 1] and [r["n_local"] for r in res] == [62, 65]
    assert res[0]["one"] == res[0]["both"] == res[1]["both"] == res[1]["one"]
    real, gen = O.cluster_feats(257, 192, 0.0, 1), O.cluster_feats(130, 192, 0.6, 2)
    kept = torch.cat([torch.arange(0, 130, 2)[:-3], torch.arange(1, 130, 2)])
    want = P.prdc(_fs(real, dev), _fs(gen[kept.sort().values], dev), k=3)
    assert res[0]["sharded"] == res[1]["sharded"] == want


def test_calc_prdc_is_prdc_on_the_engines_features(dev, tmp_path):
    from naturaldiffusion_amd import CIFAR10NaturalInference as M
    from naturaldiffusion_amd import prdc as P
    from naturaldiffusion_amd.inception import InceptionEngine
    from naturaldiffusion_amd.synth import synthetic_inception_flat
    inc = InceptionEngine(synthetic_inception_flat(0), max_batch=50, device=dev)
    g = torch.Generator().manual_seed(4)
    base = torch.rand(8, 8, 8, 3, generator=g)

    def images(n, noise):                                      # smooth 32 x 32 pictures around eight prototypes: not all alike, not all apart
        up = torch.nn.functional.interpolate(base[torch.randint(0, 8, (n,), generator=g)].permute(0, 3, 1, 2), size=32, mode="bilinear")
        return ((up + noise * torch.randn(n, 3, 32, 32, generator=g)).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    real_imgs, gen_imgs = images(500, 0.05), images(600, 0.08)
    real = M.get_features(real_imgs, inc, dev)
    assert real.is_cuda and real.dtype == torch.float32 and tuple(real.shape) == (500, 2048)
    assert np.array_equal(real.cpu().numpy().astype(np.float64), M.get_activation(real_imgs, inc, 2048, dev))
    want = P.prdc(real, M.get_features(gen_imgs, inc, dev), k=3)
    assert M.calc_prdc(gen_imgs, real.cpu().numpy(), dev, model=inc, k=3) == want
    np.save(tmp_path / "pool3.npy", real.cpu().numpy())
    assert M.calc_prdc(gen_imgs.to(dev), tmp_path / "pool3.npy", dev, model=inc, k=3) == want
    assert M.calc_prdc_sharded(gen_imgs, str(tmp_path / "pool3.npy"), dev, model=inc, k=3) == want
    assert all(0.0 <= want[key] <= 1.0 for key in ("precision", "recall", "coverage")) and want["density"] >= 0.0
