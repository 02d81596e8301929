"""Inception Score on the GPU (include/natinf_is.h; naturaldiffusion_amd/iscore.py) against tests/is_oracle.py: the row statistics and the score within the
derived bounds of fp64, the same bytes for any split of the rows and for ranges taken in place, the chunk boundary of the staged logits, offsets past 2^31,
the splits protocol, two ranks and the public path.  The bounds (is_oracle's docstring) are derived from the distance kernels' band, not measured on this
code; every case first asserts on the fp64 oracle that its inputs let the comparison decide something."""
import math

import pytest
import torch

import is_oracle as IO
import prdc_oracle as O

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope="module")
def dev():
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _case(n, C, d):
    """inputs on the host, computed once, never modified"""
    if (n, C, d) not in _cache:
        _cache[(n, C, d)] = IO.case(n, C, d)
    return _cache[(n, C, d)]


def _fs(x, dev):
    from naturaldiffusion_amd import prdc as P
    return P.FeatureSet(x, device=dev)


def _head(cs, dev, bias=True):
    from naturaldiffusion_amd import iscore as I
    return I.ClassifierHead(cs["W"], cs["b"] if bias else None, device=dev)


def _within(got, ref, bound):
    return bool(((got - ref).abs() <= bound).all())


def _share(got, ref, bound):
    return float(((got - ref).abs() / bound).max())


CASES = [(130, 1008, 2048), (70, 1008, 64), (300, 257, 192), (257, 130, 64), (64, 128, 64), (1, 1, 64), (3, 2, 64)]


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("n,C,d", CASES)
def test_row_stats_and_score_against_fp64(dev, n, C, d, bias):
    """1008 classes end 112 columns into the eighth tile, 257 one column into the third, 130 two into the second, 128 is one whole tile; 130, 70, 300 and 257
    rows are off the 64-row block.  Without the bias nothing offsets the logits, so the z = 0 padding condition is the biased cases' alone; with one row the
    score is 1 whatever the head, so there the score is compared without a resolution condition."""
    from naturaldiffusion_amd import iscore as I
    cs = _case(n, C, d)
    a, W, b = cs["a"], cs["W"], cs["b"] if bias else None
    B, z = IO.bounds(a, W, b), IO.logits(a, W, b)
    # ---- the conditions, on the fp64 oracle ----
    resolved = B["gap"] >= 100 * B["E"]
    assert float(resolved.double().mean()) >= 0.9
    planted_rows = [r for _, r in cs["planted"]]
    for c, r in cs["planted"]:
        assert int(B["top"][r]) == c and bool(resolved[r]), (c, r)
        assert float((IO.lse_without(z, c)[r] - B["lse"][r]).abs()) >= 100 * float(B["lse_bound"][r]), (c, r)
    non = torch.ones(n, dtype=torch.bool)
    non[planted_rows] = False
    if bias:
        assert bool(((IO.lse_with_zero_column(z) - B["lse"]).abs() >= 100 * B["lse_bound"])[non].all())
    if n > 1:
        assert B["log_is"] >= 100 * B["log_is_bound"], (B["log_is"], B["log_is_bound"])
    # ---- the device ----
    fs, head = _fs(a, dev), _head(cs, dev, bias)
    h, lse, top, q = (v.cpu() for v in I.row_stats(fs, None, head))
    assert h.dtype == lse.dtype == torch.float64 and top.dtype == torch.int32 and q.dtype == torch.int64
    assert tuple(h.shape) == tuple(lse.shape) == tuple(top.shape) == (n,) and tuple(q.shape) == (C,)
    res = I.inception_score(fs, head, group=I.LOCAL)
    # the plain statements in fp32 on the same device
    zt = a.to(dev) @ W.to(dev).t() + (b.to(dev) if bias else 0.0)
    lpt = torch.log_softmax(zt, 1)
    ht, lset, pt = (lpt.exp() * lpt).sum(1).cpu().double(), torch.logsumexp(zt, 1).cpu().double(), lpt.exp().mean(0).cpu().double()
    score_t = float(ht.mean() - (pt[pt > 0] * pt[pt > 0].log()).sum())
    print(f"is ({n}, {C}, {d}) {'bias' if bias else 'no bias'}: lse kernel {_share(lse, B['lse'], B['lse_bound']):.3e} of the bound, torch fp32 "
          f"{_share(lset, B['lse'], B['lse_bound']):.3e}; h kernel {_share(h, B['h'], B['h_bound']):.3e}, torch fp32 {_share(ht, B['h'], B['h_bound']):.3e}; "
          f"log IS {res['log_is'][0]!r} fp64 {B['log_is']!r} kernel {abs(res['log_is'][0] - B['log_is']) / B['log_is_bound']:.3e} of the bound, torch fp32 "
          f"{abs(score_t - B['log_is']) / B['log_is_bound']:.3e}; Q kernel {_share(q.double(), B['q'], B['q_bound']):.3e}; "
          f"tops equal {float((top.long() == B['top']).double().mean()):.3f}")
    assert _within(lse, B["lse"], B["lse_bound"]), _share(lse, B["lse"], B["lse_bound"])
    assert _within(h, B["h"], B["h_bound"]), _share(h, B["h"], B["h_bound"])
    assert bool((top.long() == B["top"])[resolved].all())
    assert _within(q.double(), B["q"], B["q_bound"]), _share(q.double(), B["q"], B["q_bound"])
    assert bool((q >= 0).all()) and abs(int(q.sum()) - n * (1 << 42)) <= n * C             # every row's q add up to 2^42 within C / 2
    assert res["n"] == n and res["splits"] == 1 and res["std"] is None and res["is"] == math.exp(res["log_is"][0])
    assert abs(res["log_is"][0] - B["log_is"]) <= B["log_is_bound"], (res["log_is"][0], B["log_is"], B["log_is_bound"])
    assert res["log_is"][0] == I.log_score(h, q, n)


def test_refusals_and_empty_ranges(dev):
    from naturaldiffusion_amd import iscore as I
    cs = _case(64, 128, 64)
    fs, head = _fs(cs["a"], dev), _head(cs, dev)
    with pytest.raises(ValueError, match="feature width"):
        I.row_stats(_fs(O.cluster_feats(3, 192, 0.0, 1), dev), None, head)
    with pytest.raises(ValueError, match="range"):
        I.row_stats(fs, range(60, 65), head)
    with pytest.raises(ValueError, match="range"):
        I.row_stats(fs, range(0, 64, 2), head)
    with pytest.raises(ValueError, match="devices"):
        elsewhere = head.without_bias()                                # (a copy)
        elsewhere.device = torch.device("cpu")
        I.row_stats(fs, None, elsewhere)
    with pytest.raises(ValueError, match="0 rows"):
        I.inception_score(fs, head, splits=65, group=I.LOCAL)
    with pytest.raises(ValueError, match="bias"):
        I.ClassifierHead(cs["W"], cs["b"][:5], device=dev)
    h, lse, top, q = I.row_stats(fs, range(7, 7), head)
    assert h.numel() == lse.numel() == top.numel() == 0 and tuple(q.shape) == (128,) and int(q.abs().sum()) == 0


def test_splits_of_the_rows_give_the_bytes_of_the_whole_call(dev):
    from naturaldiffusion_amd import iscore as I
    from naturaldiffusion_amd import prdc as P
    cs = _case(300, 257, 192)
    a = cs["a"]
    fs, head = _fs(a, dev), _head(cs, dev)
    whole = I.row_stats(fs, range(300), head)

    def same(parts):
        for k in range(3):                                             # h, lse, top: the same bytes
            assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), k
        assert torch.equal(torch.stack([p[3] for p in parts]).sum(0), whole[3])          # the class sums: the same integers

    same([I.row_stats(fs, r, head) for r in (range(0, 64), range(64, 193), range(193, 300))])
    for world in (2, 3):
        same([I.row_stats(fs, P.row_slice(300, r, world), head) for r in range(world)])
    same([I.row_stats(fs, range(300), head)])                          # and on every run
    # a row range taken in place equals a copy of those rows
    got = I.row_stats(fs, range(64, 193), head)
    copy = I.row_stats(_fs(a[64:193].clone(), dev), None, head)
    assert all(torch.equal(g, c) for g, c in zip(got, copy))
    assert torch.equal(got[0], whole[0][64:193]) and not torch.equal(got[3], whole[3])
    # another order of the rows: the same class sums, the rows' values moved with them
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(5))
    moved = I.row_stats(_fs(a[perm], dev), None, head)
    assert torch.equal(moved[3], whole[3])
    for k in range(3):
        assert torch.equal(moved[k].cpu(), whole[k].cpu()[perm]), k
    assert I.inception_score(_fs(a[perm], dev), head, group=I.LOCAL) == I.inception_score(fs, head, group=I.LOCAL)


def test_the_chunk_boundary_of_the_staged_logits(dev):
    """8,200 rows are one chunk of 8,192 and one of 8: rows 8,190 to 8,199 (NATINF_IS_CHUNK_ROWS - 2 to + 7) equal the same rows computed alone"""
    from naturaldiffusion_amd import iscore as I
    cs = _case(257, 130, 64)
    a = O.cluster_feats(8200, 64, 0.6, 2)
    fs, head = _fs(a, dev), _head(cs, dev)
    whole = I.row_stats(fs, None, head)
    tail = I.row_stats(fs, range(8190, 8200), head)
    for k in range(3):
        assert torch.equal(tail[k], whole[k][8190:8200]), k
    assert torch.equal(I.row_stats(fs, range(0, 8190), head)[3] + tail[3], whole[3])
    B = IO.bounds(a[8100:], cs["W"], cs["b"])
    assert _within(whole[1].cpu()[8100:], B["lse"], B["lse_bound"]) and _within(whole[0].cpu()[8100:], B["h"], B["h_bound"])
    assert _within(I.row_stats(fs, range(8100, 8200), head)[3].cpu().double(), B["q"], B["q_bound"])


def test_offsets_past_two_to_the_31(dev):
    """524,800 x 2048 rows: the third plane starts 2.1e9 elements into the buffer; 96 rows at 524,700 are taken in place against the (1008, 2048) head"""
    from naturaldiffusion_amd import iscore as I
    from naturaldiffusion_amd import prdc as P
    n, d, s = 524800, 2048, 524700
    g = torch.Generator(device=dev).manual_seed(3)
    Wm = torch.randn(6, d, generator=g, device=dev)
    x = torch.randn(n, d, generator=g, device=dev).mul_(0.3)
    x.addmm_(torch.randn(n, 6, generator=g, device=dev), Wm).relu_().mul_(0.5)
    fs = P.FeatureSet(x, device=dev)
    assert 2 * n * d > 2 ** 31
    cs = _case(130, 1008, 2048)
    head = _head(cs, dev)
    rows = x[s:s + 96].cpu()
    del x
    got = I.row_stats(fs, range(s, s + 96), head)
    copy = I.row_stats(P.FeatureSet(rows.clone(), device=dev), None, head)
    assert all(torch.equal(g_, c_) for g_, c_ in zip(got, copy))
    B = IO.bounds(rows, cs["W"], cs["b"])
    assert _within(got[1].cpu(), B["lse"], B["lse_bound"]), _share(got[1].cpu(), B["lse"], B["lse_bound"])
    assert _within(got[0].cpu(), B["h"], B["h_bound"]), _share(got[0].cpu(), B["h"], B["h_bound"])
    assert _within(got[3].cpu().double(), B["q"], B["q_bound"])


def test_the_splits_protocol(dev):
    from naturaldiffusion_amd import iscore as I
    cs = _case(257, 130, 64)
    fs, head = _fs(cs["a"], dev), _head(cs, dev)
    ref = IO.score_splits(cs["a"], cs["W"], cs["b"], 3)
    assert min(v / e for v, e in zip(ref["log_is"], ref["log_is_bounds"])) >= 100 and ref["std"] >= 100 * ref["std_bound"], ref
    got = I.inception_score(fs, head, splits=3, group=I.LOCAL)
    print(f"is splits: {got} fp64 {ref}")
    assert got["splits"] == 3 and got["n"] == 257 and len(got["log_is"]) == 3
    for v, r, e in zip(got["log_is"], ref["log_is"], ref["log_is_bounds"]):
        assert abs(v - r) <= e, (v, r, e)
    assert abs(got["is"] - ref["is"]) <= ref["is_bound"] and abs(got["std"] - ref["std"]) <= ref["std_bound"]
    # a split is the score of its rows
    for k, b in enumerate(I.split_bounds(257, 3)):
        assert I.inception_score(_fs(cs["a"][b.start:b.stop].clone(), dev), head, group=I.LOCAL)["log_is"][0] == got["log_is"][k]
    one = I.inception_score(fs, head, splits=1, group=I.LOCAL)
    assert one["std"] is None and one["splits"] == 1 and one == I.inception_score(cs["a"].to(dev), head, group=I.LOCAL)          # from a tensor


_RANK_SCRIPT = r"""
import os, sys, json
import torch, torch.distributed as dist
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
import is_oracle as IO
from naturaldiffusion_amd import CIFAR10NaturalInference as M
from naturaldiffusion_amd import iscore as I
from naturaldiffusion_amd import prdc as P
dev = torch.device("cuda:0")
cs = IO.case(257, 130, 64)
feats = cs["a"][:130].contiguous()
head = I.ClassifierHead(cs["W"], cs["b"], device=dev)
idx = torch.arange(rank, 130, world) if rank else torch.arange(rank, 130, world)[:-3]      # ragged shares: 62 and 65 rows, 127 in all
kept = torch.cat([torch.arange(0, 130, 2)[:-3], torch.arange(1, 130, 2)])                   # the gathered order: rank 0's rows, then rank 1's
one = {{s: I.inception_score(P.FeatureSet(feats[kept], device=dev), head, splits=s, group=I.LOCAL) for s in (1, 3)}}      # no collective
both = {{s: I.inception_score(P.FeatureSet(feats[idx], device=dev), head, splits=s) for s in (1, 3)}}                    # every rank its own rows


class Lookup:                                                                 # stands for the Inception engine: image i is the picture of feature row i
    max_batch = 50

    def __call__(self, imgs):
        return feats.to(dev)[imgs[:, 0, 0, 0].long().to(dev)]


imgs = torch.zeros(130, 2, 2, 3, dtype=torch.uint8)
imgs[:, 0, 0, 0] = torch.arange(130, dtype=torch.uint8)
mine = imgs[idx]
sharded = {{s: M.calc_is_sharded(mine, dev, model=Lookup(), head=head, splits=s) for s in (1, 3)}}
nobias = M.calc_is_sharded(mine, dev, model=Lookup(), head=head, splits=3, bias=False)
local = M.calc_is(mine, dev, model=Lookup(), head=head)                        # this rank's images alone, though a group exists
with open({out!r} + f"/rank{{rank}}.json", "w") as fh:                          # (two ranks' lines on one stdout can run into each other)
    json.dump(dict(rank=rank, one=one, both=both, sharded=sharded, nobias=nobias, local=local, n_local=len(mine)), fh)
dist.destroy_process_group()
"""


def test_two_ranks_give_one_ranks_numbers(dev, tmp_path):
    """inception_score() in a process group of two (gloo, both ranks on cuda:0) on ragged shares of the rows returns, on both ranks, the dict one process
    returns on the gathered order, byte for byte; so does calc_is_sharded; group=LOCAL scores a rank's own rows"""
    import json, os, socket, subprocess, sys
    from pathlib import Path
    from naturaldiffusion_amd import iscore as I
    root = Path(__file__).resolve().parent.parent
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT.format(root=str(root), out=str(tmp_path)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    with socket.socket() as s:                                        # a port that is free now: another copy of the suite on this host takes another
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = [json.loads((tmp_path / f"rank{r}.json").read_text()) for r in (0, 1)]
    assert [r["rank"] for r in res] == [0, 1] and [r["n_local"] for r in res] == [62, 65]
    assert res[0]["one"] == res[0]["both"] == res[1]["both"] == res[1]["one"] == res[0]["sharded"] == res[1]["sharded"]
    assert res[0]["one"]["3"]["std"] > 0 and res[0]["one"]["1"]["std"] is None and res[0]["one"]["3"]["n"] == 127
    cs = _case(257, 130, 64)
    feats, head = cs["a"][:130], _head(cs, dev)
    shares = [torch.arange(0, 130, 2)[:-3], torch.arange(1, 130, 2)]
    kept = torch.cat(shares)
    for s in (1, 3):
        assert res[0]["one"][str(s)] == I.inception_score(_fs(feats[kept], dev), head, splits=s, group=I.LOCAL), s
    assert res[0]["nobias"] == res[1]["nobias"] == I.inception_score(_fs(feats[kept], dev), head.without_bias(), splits=3, group=I.LOCAL)
    assert res[0]["nobias"] != res[0]["one"]["3"]
    for r in (0, 1):
        assert res[r]["local"] == I.inception_score(_fs(feats[shares[r]], dev), head, group=I.LOCAL), r


def test_calc_is_is_the_score_of_the_engines_features(dev):
    from naturaldiffusion_amd import CIFAR10NaturalInference as M
    from naturaldiffusion_amd import iscore as I
    from naturaldiffusion_amd.inception import InceptionEngine
    from naturaldiffusion_amd.synth import synthetic_inception_flat, synthetic_inception_head
    inc = InceptionEngine(synthetic_inception_flat(0), max_batch=50, device=dev)
    head = I.ClassifierHead(*synthetic_inception_head(0), device=dev)
    g = torch.Generator().manual_seed(4)
    base = torch.rand(8, 8, 8, 3, generator=g)

    def images(n, noise):                                      # smooth 32 x 32 pictures around eight prototypes: not all alike, not all apart
        up = torch.nn.functional.interpolate(base[torch.randint(0, 8, (n,), generator=g)].permute(0, 3, 1, 2), size=32, mode="bilinear")
        return ((up + noise * torch.randn(n, 3, 32, 32, generator=g)).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    images(500, 0.05)                                          # (the generator's state where test_calc_kid_is_kid_on_the_engines_features makes its 600)
    imgs = images(600, 0.08)
    feats = M.get_features(imgs, inc, dev)
    want = I.inception_score(feats, head, group=I.LOCAL)
    assert want["n"] == 600 and want["std"] is None and math.isfinite(want["is"]) and 1.0 <= want["is"] <= 1008.0
    assert M.calc_is(imgs, dev, model=inc, head=head) == want
    assert M.calc_is(imgs.to(dev), dev, model=inc, head=head) == want
    assert M.calc_is_sharded(imgs, dev, model=inc, head=head) == want
    plain = I.inception_score(feats, head.without_bias(), group=I.LOCAL)
    assert M.calc_is(imgs, dev, model=inc, head=head, bias=False) == plain and plain != want and 1.0 <= plain["is"] <= 1008.0
    ten = I.inception_score(feats, head, splits=10, group=I.LOCAL)
    assert M.calc_is(imgs, dev, model=inc, head=head, splits=10) == ten
    assert ten["splits"] == 10 and len(ten["log_is"]) == 10 and ten["std"] > 0.0 and all(1.0 <= math.exp(v) <= 1008.0 for v in ten["log_is"])
