"""Nearest neighbours on the GPU (include/natinf_nn.h; naturaldiffusion_amd/neighbours.py): distances and indices against an independent exact oracle in
pixel space, ties, the library's own distance matrix and radii byte for byte, the smallest legal column counts, the same bytes for any split of the rows,
and the job layer.

The pixel-space oracle is exact: a uint8 value is exact in the first bf16 plane (the other two are zero), a product of two is below 2^16, 64 of them
add up below 2^22 in the fp32 accumulator, and everything behind it is fp64 on integers far below 2^53.  So the kernel's d2 must EQUAL numpy's int64 sum of
squared differences, and its indices a stable argsort's."""
import struct

import numpy as np
import pytest
import torch

import prdc_oracle as O

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope="module")
def dev():
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _pixel_d2(a, b):
    """int64 [na, nb]: the sum of squared differences of uint8 images, one row of the table at a time"""
    a, b = a.reshape(len(a), -1).astype(np.int64), b.reshape(len(b), -1).astype(np.int64)
    return np.stack([((r[None, :] - b) ** 2).sum(1) for r in a])


def _first_k(d2, k, self_offset=-1, row0=0):
    """(d2, idx) [n, k] of a distance table: the first k of a stable sort of every row, column self_offset + row0 + i of row i left out"""
    d2 = np.array(d2, dtype=np.float64)
    if self_offset >= 0:
        d2[np.arange(len(d2)), self_offset + row0 + np.arange(len(d2))] = np.inf
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d2, idx, 1), idx


def _images(n, hw, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)


def _pixel_set(imgs, dev):
    from naturaldiffusion_amd import neighbours as N
    from naturaldiffusion_amd.prdc import FeatureSet
    return FeatureSet(N.pixel_features(torch.from_numpy(imgs), dev), device=dev)


def _same_bytes(a, b):
    a, b = torch.as_tensor(a).cpu().contiguous(), torch.as_tensor(b).cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


def _cifar_pair():
    if "cifar" not in _cache:
        a, b = _images(70, 32, 11), _images(300, 32, 12)
        _cache["cifar"] = (a, b, _pixel_d2(a, b))
    return _cache["cifar"]


@pytest.mark.parametrize("k", [1, 3, 8])
def test_pixel_space_equals_the_int64_oracle(dev, k):
    """d = 3,072, 70 rows (one row block and six rows) x 300 columns (two tiles and 44 columns, three column ranges)"""
    from naturaldiffusion_amd import neighbours as N
    a, b, table = _cifar_pair()
    d2, idx = N.nearest(_pixel_set(a, dev), _pixel_set(b, dev), k=k)
    assert d2.dtype == torch.float64 and idx.dtype == torch.int64 and tuple(d2.shape) == (70, k) == tuple(idx.shape) and d2.is_cuda and idx.is_cuda
    want_d2, want_idx = _first_k(table, k)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(d2.cpu().numpy(), want_d2)


def _tie_case():
    """600 columns (five tiles, five column ranges): 60 distinct 8 x 8 images, ten byte copies of each at shuffled places; 40 rows, the first 12 of them
    copies of distinct images 0..11"""
    if "ties" not in _cache:
        rng = np.random.default_rng(21)
        distinct = _images(60, 8, 22)
        which = rng.permutation(np.repeat(np.arange(60), 10))
        rows = _images(40, 8, 23)
        rows[:12] = distinct[:12]
        _cache["ties"] = (rows, distinct[which], which, _pixel_d2(rows, distinct[which]))
    return _cache["ties"]


def test_ties_come_out_in_ascending_column_order(dev):
    from naturaldiffusion_amd import neighbours as N
    rows, cols, which, table = _tie_case()
    rs, cs = _pixel_set(rows, dev), _pixel_set(cols, dev)
    spread = 0
    for k in (1, 3, 8):
        d2, idx = (v.cpu().numpy() for v in N.nearest(rs, cs, k=k))
        want_d2, want_idx = _first_k(table, k)
        assert np.array_equal(idx, want_idx) and np.array_equal(d2, want_d2), k
        for i in range(12):                                          # a copy's neighbours are its k lowest copies among the columns, at distance 0
            copies = np.flatnonzero(which == i)
            assert (d2[i] == 0).all() and np.array_equal(idx[i], copies[:k]), (k, i)
            if k == 8:
                spread += len(set(copies[:8] % 4)) >= 3 and len(set(copies[:8] // 128)) >= 3
        # every row's nearest image exists ten times: all k slots are ties, in ascending order
        assert (d2 == d2[:, :1]).all() and (np.diff(idx, axis=1) > 0).all(), k
    assert spread >= 6, "the copies do not spread over the column classes (j mod 4) and the 128-column tiles"


@pytest.mark.parametrize("d", [64, 2048])
def test_equals_the_librarys_own_matrix_and_radii(dev, d):
    """fp32 features, 200 x 700: (d2, idx) is the first k of a stable sort of natinf_prdc_debug_dist2's rows, byte for byte, and the last column is
    natinf_prdc_knn_radius's"""
    from naturaldiffusion_amd import neighbours as N
    from naturaldiffusion_amd import prdc as P
    x, y = O.cluster_feats(200, d, 0.6, 2), O.cluster_feats(700, d, 0.0, 1)
    y[311], y[40], y[699] = y[5], y[5], x[17]                        # equal columns, and a column that is a row
    rows, cols = P.FeatureSet(x, device=dev), P.FeatureSet(y, device=dev)
    for so in (-1, 0, 37, 500):                                      # nothing left out; column so + i left out of row i
        table = P.debug_dist2(rows, cols, so).cpu().numpy()
        for k in (1, 5, 8):
            d2, idx = N.nearest(rows, cols, k=k, self_offset=so)
            want_d2, want_idx = _first_k(table, k)                   # (the table holds +inf at the left-out column)
            assert np.array_equal(idx.cpu().numpy(), want_idx), (so, k)
            assert _same_bytes(d2, want_d2), (so, k)
            assert _same_bytes(d2[:, k - 1], P._knn(rows, range(200), cols, k, so)), (so, k)
    # rows [s, s + 200) of a set against the whole set, itself left out
    s = 450
    part = P.FeatureSet(y[s:s + 200], device=dev)
    table = P.debug_dist2(part, cols, s).cpu().numpy()
    assert np.isinf(table[np.arange(200), s + np.arange(200)]).all()
    for k in (1, 3, 8):
        d2, idx = N.nearest(cols, cols, k=k, row_range=range(s, s + 200), self_offset=0)
        want_d2, want_idx = _first_k(table, k)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and _same_bytes(d2, want_d2), k
        assert not (idx.cpu().numpy() == (s + np.arange(200))[:, None]).any()
        assert _same_bytes(d2[:, k - 1], P.knn_radii(cols, k, range(s, s + 200))), k
        d2p, idxp = N.nearest(part, cols, k=k, self_offset=s)        # the same rows as a set of their own
        assert _same_bytes(d2p, d2) and torch.equal(idxp, idx), k


@pytest.mark.parametrize("k", [1, 4, 8])
def test_smallest_legal_column_counts(dev, k):
    from naturaldiffusion_amd import neighbours as N
    b = _images(65, 8, 31)
    b[3] = b[0]
    cols_all = _pixel_set(b, dev)
    # one row, k + 1 columns, one of them left out: every other column comes back, sorted
    few = _pixel_set(b[:k + 1], dev)
    for so in (0, k):
        a = b[so:so + 1] if so == 0 else _images(1, 8, 32)
        d2, idx = N.nearest(_pixel_set(a, dev), few, k=k, self_offset=so)
        want_d2, want_idx = _first_k(_pixel_d2(a, b[:k + 1]), k, so)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(d2.cpu().numpy(), want_d2), so
        assert sorted(idx[0].tolist()) == [j for j in range(k + 1) if j != so]
    # k + 1 rows of the set against itself: row i gets every column but i
    d2, idx = N.nearest(few, few, k=k, self_offset=0)
    want_d2, want_idx = _first_k(_pixel_d2(b[:k + 1], b[:k + 1]), k, 0)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(d2.cpu().numpy(), want_d2)
    # 65 rows (one full row block and one row): k columns and nothing left out; 65 columns, the fewest that leave one out of every row
    a = _images(65, 8, 33)
    d2, idx = N.nearest(_pixel_set(a, dev), _pixel_set(b[:k], dev), k=k)
    want_d2, want_idx = _first_k(_pixel_d2(a, b[:k]), k)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(d2.cpu().numpy(), want_d2)
    d2, idx = N.nearest(cols_all, cols_all, k=k, self_offset=0)
    want_d2, want_idx = _first_k(_pixel_d2(b, b), k, 0)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(d2.cpu().numpy(), want_d2)
    with pytest.raises(ValueError, match="prdc: "):                   # too few columns (k = 8: beyond the list)
        N.nearest(few, few, k=k + 1, self_offset=0)


def test_any_split_of_the_rows_gives_the_same_bytes(dev):
    """2,600 columns are 21 tiles: 2,100 rows in one call sweep them in 15 column ranges, 1,000 and 1,100 rows in 21, as does a single row.  The columns are
    260 images ten times over, so every slot of every row is a tie that the ranges' merge has to order."""
    from naturaldiffusion_amd import neighbours as N
    rng = np.random.default_rng(41)
    distinct = _images(260, 8, 42)
    cols = _pixel_set(distinct[rng.permutation(np.repeat(np.arange(260), 10))], dev)
    rows_u8 = _images(2100, 8, 43)
    rows_u8[::7] = distinct[rng.integers(0, 260, len(rows_u8[::7]))]
    rows = _pixel_set(rows_u8, dev)
    k = 8
    d2, idx = N.nearest(rows, cols, k=k)
    assert (d2 == d2[:, :1]).all() and (idx[:, 1:] > idx[:, :-1]).all() and int((d2[:, 0] == 0).sum()) == 300
    lo, hi = N.nearest(rows, cols, k=k, row_range=range(0, 1000)), N.nearest(rows, cols, k=k, row_range=range(1000, 2100))
    assert _same_bytes(torch.cat([lo[0], hi[0]]), d2) and torch.equal(torch.cat([lo[1], hi[1]]), idx)
    for i in (0, 1, 63, 64, 999, 1000, 2099):
        one = N.nearest(rows, cols, k=k, row_range=range(i, i + 1))
        assert _same_bytes(one[0], d2[i:i + 1]) and torch.equal(one[1], idx[i:i + 1]), i
    # the oracle on the single rows
    table = _pixel_d2(rows_u8[[0, 63, 64, 2099]], distinct)
    assert np.array_equal(d2[[0, 63, 64, 2099], 0].cpu().numpy(), table.min(1).astype(np.float64))
    empty = N.nearest(rows, cols, k=k, row_range=range(5, 5))
    assert tuple(empty[0].shape) == (0, k) == tuple(empty[1].shape)


_RANK_SCRIPT = r"""
import os, sys
import numpy as np
import torch, torch.distributed as dist
sys.path.insert(0, {root!r})
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
from naturaldiffusion_amd import CIFAR10NaturalInference as M
dev = torch.device("cuda:0")
data = np.load({out!r} + "/images.npz")
gen, ref = torch.from_numpy(data["gen"]), torch.from_numpy(data["ref"])
mine = gen[:23] if rank == 0 else gen[23:]                                    # ragged shares in rank order: 23 and 41 images
res = M.calc_nearest_sharded(mine, ref, dev, space="pixel", k=3)
np.savez({out!r} + f"/rank{{rank}}.npz", d2=res["d2"], idx=res["idx"], summary=np.array([res["summary"][key] for key in ("n", "min", "median", "mean", "copies")]))
dist.destroy_process_group()
"""


def test_two_ranks_give_one_ranks_table(dev, tmp_path):
    """calc_nearest_sharded in a process group of two (gloo, both ranks on cuda:0): ragged shares of the images, every rank returns the whole table in rank
    order -- the table of one process on all the images"""
    import os, socket, subprocess, sys
    from pathlib import Path
    from naturaldiffusion_amd import CIFAR10NaturalInference as M
    ref, gen = _images(300, 8, 61), _images(64, 8, 62)
    gen[[2, 30, 63]] = ref[[7, 7, 250]]
    np.savez(tmp_path / "images.npz", gen=gen, ref=ref)
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT.format(root=str(Path(__file__).resolve().parent.parent), out=str(tmp_path)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    with socket.socket() as s:                                        # a port that is free now
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    want = M.calc_nearest(torch.from_numpy(gen), torch.from_numpy(ref), dev, space="pixel", k=3)
    assert want["summary"]["copies"] == 3 and want["idx"][30, 0] == 7
    for r in (0, 1):
        got = np.load(tmp_path / f"rank{r}.npz")
        assert np.array_equal(got["d2"], want["d2"]) and np.array_equal(got["idx"], want["idx"]), r
        assert got["summary"].tolist() == [want["summary"][key] for key in ("n", "min", "median", "mean", "copies")], r


def _png_size(path):
    head = open(path, "rb").read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR"
    return struct.unpack(">II", head[16:24])


def test_job_layer(dev, tmp_path):
    from naturaldiffusion_amd import CIFAR10NaturalInference as M
    from naturaldiffusion_amd import neighbours as N
    from naturaldiffusion_amd import prdc as P
    from naturaldiffusion_amd.inception import InceptionEngine
    from naturaldiffusion_amd.synth import synthetic_inception_flat
    ref = _images(300, 32, 51)
    gen = _images(64, 32, 52)
    planted = {0: 299, 5: 128, 17: 0, 40: 131, 63: 7}
    for i, j in planted.items():
        gen[i] = ref[j]
    ref[200] = ref[131]                                              # a duplicate in the training set: the lower index is reported
    gen_t, ref_t = torch.from_numpy(gen), torch.from_numpy(ref)
    # pixel space
    res = M.calc_nearest(gen_t, ref_t, dev, space="pixel", k=3)
    assert isinstance(res["d2"], np.ndarray) and res["d2"].dtype == np.float64 and res["idx"].dtype == np.int64 and res["d2"].shape == (64, 3) == res["idx"].shape
    want_d2, want_idx = _first_k(_pixel_d2(gen, ref), 3)
    assert np.array_equal(res["idx"], want_idx) and np.array_equal(res["d2"], want_d2)
    for i, j in planted.items():
        assert res["idx"][i, 0] == j and res["d2"][i, 0] == 0.0, i
    assert res["idx"][40, 1] == 200 and res["d2"][40, 1] == 0.0
    assert res["summary"] == N.summary(want_d2) and res["summary"]["copies"] == len(planted) and res["summary"]["n"] == 64
    assert res["space"] == "pixel" and res["k"] == 3
    sharded = M.calc_nearest_sharded(gen_t.to(dev), ref, dev, space="pixel", k=3, group=None)
    assert np.array_equal(sharded["d2"], res["d2"]) and np.array_equal(sharded["idx"], res["idx"]) and sharded["summary"] == res["summary"]
    # the Inception features FID is computed from
    inc = InceptionEngine(synthetic_inception_flat(0), max_batch=50, device=dev)
    ref_feats = M.get_features(ref_t, inc, dev)
    res3 = M.calc_nearest(gen_t, ref_feats.cpu().numpy(), dev, space="pool3", k=2, model=inc)
    d2, idx = N.nearest(P.FeatureSet(M.get_features(gen_t, inc, dev), device=dev), P.FeatureSet(ref_feats, device=dev), k=2)
    assert np.array_equal(res3["d2"], d2.cpu().numpy()) and np.array_equal(res3["idx"], idx.cpu().numpy()) and res3["summary"] == N.summary(d2)
    assert res3["idx"].min() >= 0 and res3["idx"].max() < 300 and (np.diff(res3["d2"], axis=1) >= 0).all()
    np.save(tmp_path / "pool3.npy", ref_feats.cpu().numpy())
    sharded3 = M.calc_nearest_sharded(gen_t, tmp_path / "pool3.npy", dev, space="pool3", k=2, model=inc)
    assert np.array_equal(sharded3["d2"], res3["d2"]) and np.array_equal(sharded3["idx"], res3["idx"]) and sharded3["summary"] == res3["summary"]
    with pytest.raises(ValueError, match="space"):
        M.calc_nearest(gen_t, ref_t, dev, space="latent")
    with pytest.raises(FileNotFoundError, match="nearest: blocked"):
        M.calc_nearest(gen_t, tmp_path / "absent.npy", dev, space="pool3", model=inc)
    # the sheet: 10 lines of one image and its 3 neighbours, 32 x 32 tiles with 2 pixels of padding
    M.save_neighbour_sheet(gen_t, ref_t, res["idx"], tmp_path / "sheet.png", count=10)
    assert _png_size(tmp_path / "sheet.png") == (2 + 4 * 34, 2 + 10 * 34)
