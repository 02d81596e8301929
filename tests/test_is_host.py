"""Host side of the Inception Score (include/natinf_is.h; naturaldiffusion_amd/iscore.py): every refusal of the two entries, the workspace query, the split
bounds and the host formula by hand and against tests/is_oracle.py, the head loader, the synthetic head, the import without the library, and the oracle
against itself.  No GPU."""
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

import is_oracle as IO
from naturaldiffusion_amd import _lib
from naturaldiffusion_amd import iscore as I

EINVAL = -1
L = _lib.lib

# never dereferenced: every call below must be refused before anything is configured or launched
PTR = 0x1000            # 256-byte aligned, non-null

GPU_CASES = [(130, 1008, 2048), (70, 1008, 64), (300, 257, 192), (257, 130, 64), (64, 128, 64), (1, 1, 64), (3, 2, 64)]       # tests/test_gpu_is.py's


def _stats(rp=PTR, rs=None, n_rows=4, hp=PTR, hs=None, n_classes=8, d=64, bias=None, h=PTR, lse=PTR, top=PTR, sums=PTR, ws=PTR, ws_bytes=1 << 30):
    rs = max(n_rows, 0) * max(d, 0) if rs is None else rs
    hs = max(n_classes, 0) * max(d, 0) if hs is None else hs
    return L.natinf_is_row_stats(rp, rs, n_rows, hp, hs, n_classes, d, bias, h, lse, top, sums, ws, ws_bytes, None)


def test_argument_errors_are_einval():
    for d in (0, 32, 96, -64, 4096 + 64, 65536):
        assert _stats(d=d) == EINVAL and L.natinf_is_workspace_bytes(4, 8, d) == EINVAL, d
    for n in (0, -1, (1 << 20) + 1):
        assert _stats(n_rows=n) == EINVAL and L.natinf_is_workspace_bytes(n, 8, 64) == EINVAL, n
    for c in (0, -1, 4097, 1 << 20):
        assert _stats(n_classes=c) == EINVAL and L.natinf_is_workspace_bytes(4, c, 64) == EINVAL, c
    # null and misaligned pointers; lse, top and the bias may be null
    for name in ("rp", "hp", "h", "sums", "ws"):
        assert _stats(**{name: None}) == EINVAL, name
    assert _stats(rp=PTR + 8) == EINVAL and _stats(hp=PTR + 8) == EINVAL and _stats(h=PTR + 4) == EINVAL and _stats(sums=PTR + 4) == EINVAL
    assert _stats(lse=PTR + 4) == EINVAL and _stats(top=PTR + 2) == EINVAL and _stats(bias=PTR + 2) == EINVAL and _stats(ws=PTR + 16) == EINVAL
    # a plane stride holds the operand's rows at least and keeps every plane 16-byte aligned
    assert _stats(rs=4 * 64 - 8) == EINVAL and _stats(hs=8 * 64 - 8) == EINVAL and _stats(rs=0) == EINVAL and _stats(hs=-512) == EINVAL
    for off in (1, 2, 4, 12):
        assert _stats(rs=4 * 64 + off) == EINVAL and _stats(hs=8 * 64 + off) == EINVAL, off
    # a short workspace
    need = L.natinf_is_workspace_bytes(4, 8, 64)
    assert need == 4 * 128 * 8 and _stats(ws_bytes=need - 1) == EINVAL and _stats(ws_bytes=0) == EINVAL
    need = L.natinf_is_workspace_bytes(9000, 1008, 2048)
    assert _stats(n_rows=9000, n_classes=1008, d=2048, ws_bytes=need - 1) == EINVAL


def test_workspace_bytes():
    ns = [1, 2, 63, 64, 65, 1000, 4096, 8191, 8192, 8193, 50000, 65536, 1 << 20]
    cs = [1, 2, 127, 128, 129, 1008, 1024, 1025, 4096]
    b = np.array([[L.natinf_is_workspace_bytes(n, c, 2048) for c in cs] for n in ns], dtype=np.int64)
    assert (b > 0).all() and (np.diff(b, axis=0) >= 0).all() and (np.diff(b, axis=1) >= 0).all()
    for d0, d1 in ((64, 2048), (2048, 4096)):
        assert L.natinf_is_workspace_bytes(5000, 1008, d0) <= L.natinf_is_workspace_bytes(5000, 1008, d1)
    # min(n_rows, 8192) rows of ceil(C / 128) * 128 doubles: 64 MiB for the real head at any number of rows from one chunk up
    assert L.natinf_is_workspace_bytes(50000, 1008, 2048) == 64 << 20 == L.natinf_is_workspace_bytes(8192, 1008, 2048) == L.natinf_is_workspace_bytes(1 << 20, 1008, 2048)
    assert L.natinf_is_workspace_bytes(130, 130, 64) == 130 * 256 * 8 and L.natinf_is_workspace_bytes(1, 1, 64) == 128 * 8
    assert L.natinf_is_workspace_bytes(1 << 20, 4096, 4096) == 8192 * 4096 * 8


def test_row_stats_refuses_before_any_launch():
    """the Python entry's refusals are ValueErrors raised from the shapes alone: stand-ins without planes are enough"""
    class Shape:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    cpu = torch.device("cpu")
    head = Shape(d=64, classes=8, device=cpu)
    with pytest.raises(ValueError, match="feature width"):
        I.row_stats(Shape(n=4, d=128, device=cpu), None, head)
    with pytest.raises(ValueError, match="devices"):
        I.row_stats(Shape(n=4, d=64, device=torch.device("cuda:0")), None, head)
    for r in (range(-1, 3), range(2, 5), range(0, 4, 2)):
        with pytest.raises(ValueError, match="range"):
            I.row_stats(Shape(n=4, d=64, device=cpu), r, head)
    with pytest.raises(ValueError, match="rows in one call"):
        I.row_stats(Shape(n=(1 << 20) + 1, d=64, device=cpu), None, head)
    with pytest.raises(ValueError, match="classes"):
        I.ClassifierHead(torch.zeros(4097, 64))
    with pytest.raises(ValueError, match="fp32"):
        I.ClassifierHead(torch.zeros(8, 64, dtype=torch.float64))


def test_split_bounds_by_hand():
    assert I.split_bounds(10, 1) == [range(10)]
    assert I.split_bounds(10, 3) == [range(0, 3), range(3, 6), range(6, 10)]
    assert I.split_bounds(257, 3) == [range(0, 85), range(85, 171), range(171, 257)]
    assert I.split_bounds(3, 3) == [range(0, 1), range(1, 2), range(2, 3)]
    assert [(r.start, r.stop) for r in I.split_bounds(257, 3)] == IO.split_bounds(257, 3)
    assert [len(r) for r in I.split_bounds(50000, 10)] == [5000] * 10
    for n, s in ((2, 3), (0, 1), (9, 10)):
        with pytest.raises(ValueError, match="0 rows"):
            I.split_bounds(n, s)
    with pytest.raises(ValueError):
        I.split_bounds(10, 0)


def _q(p):
    return [int(v) for v in torch.round(p.double() * IO.ONE).long().sum(0).tolist()]


def test_log_score_by_hand():
    one = 1 << I.FRAC_BITS
    # uniform p over C classes in every row: IS = 1
    for n, C in ((5, 8), (64, 1024), (1, 1)):
        got = I.log_score([-math.log(C)] * n, [n * one // C] * C, n)
        assert abs(got) <= 1e-15 * (1 + math.log(C)), (n, C, got)
    # one-hot rows spread evenly over the classes: IS = C
    for n, C in ((8, 8), (24, 8), (3000, 1000)):
        got = I.log_score([0.0] * n, [(n // C) * one] * C, n)
        assert abs(got - math.log(C)) <= 1e-14, (n, C, got)
    # classes nobody has are skipped: one-hot rows over 4 of 16 classes give IS = 4
    assert abs(I.log_score(torch.zeros(8, dtype=torch.float64), torch.tensor([2 * one, 0, 0, 2 * one] * 2 + [0] * 8), 8) - math.log(4)) <= 1e-15
    # the row values in any order, as tensors or lists
    g = torch.Generator().manual_seed(0)
    p = torch.softmax(3 * torch.randn(37, 11, generator=g, dtype=torch.float64), 1)
    h = (p * p.log()).sum(1)
    got = I.log_score(h, torch.tensor(_q(p)), 37)
    assert got == I.log_score(h.flip(0).tolist(), _q(p), 37)
    assert abs(got - IO.log_score(p)) <= 1e-12, (got, IO.log_score(p))
    with pytest.raises(ValueError):
        I.log_score([0.0] * 3, [one], 4)
    with pytest.raises(ValueError):
        I.log_score([0.0], [-1, one + 1], 1)


def test_log_score_against_the_oracle_on_the_cases():
    for n, C, d in GPU_CASES:
        cs = IO.case(n, C, d)
        B = IO.bounds(cs["a"], cs["W"], cs["b"])
        got = I.log_score(B["h"], torch.tensor(_q(B["p"])), n)
        assert abs(got - B["log_is"]) <= B["log_is_bound"], (n, C, d, got, B["log_is"], B["log_is_bound"])
        assert all(abs(q - r) <= b for q, r, b in zip(_q(B["p"]), B["q"].tolist(), B["q_bound"].tolist()))


def test_module_imports_without_the_library(repo_root, tmp_path):
    """split_bounds and log_score are host code: the module imports where libnatinf.so cannot be loaded"""
    code = ("import os, sys; os.environ['NATINF_LIB'] = sys.argv[2]; sys.path.insert(0, sys.argv[1])\n"
            "from naturaldiffusion_amd import iscore as I\n"
            "assert 'naturaldiffusion_amd._lib' not in sys.modules\n"
            "print([len(r) for r in I.split_bounds(257, 3)], round(I.log_score([0.0] * 4, [1 << 43, 1 << 43], 4), 12))\n")
    p = subprocess.run([sys.executable, "-c", code, str(repo_root), str(tmp_path / "absent.so")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip() == f"[85, 86, 86] {round(math.log(2), 12)}"


def test_head_loader(tmp_path):
    from naturaldiffusion_amd.inception import head_from_state_dict, load_fid_inception_head
    g = torch.Generator().manual_seed(1)
    sd = {"Conv2d_1a_3x3.conv.weight": torch.zeros(32, 3, 3, 3), "fc.weight": torch.randn(1008, 2048, generator=g).double(), "fc.bias": torch.randn(1008, generator=g)}
    torch.save(sd, tmp_path / "ckpt.pth")
    w, b = load_fid_inception_head(tmp_path / "ckpt.pth")
    assert w.dtype == b.dtype == torch.float32 and tuple(w.shape) == (1008, 2048) and tuple(b.shape) == (1008,)
    assert torch.equal(w, sd["fc.weight"].float()) and torch.equal(b, sd["fc.bias"])
    # a pytorch_fid InceptionV3(...).state_dict() has no head
    with pytest.raises(KeyError, match="no classifier head"):
        head_from_state_dict({"blocks.0.0.conv.weight": torch.zeros(32, 3, 3, 3)})
    with pytest.raises(KeyError, match="fc.bias"):
        head_from_state_dict({"fc.weight": sd["fc.weight"]})


def test_synthetic_head():
    from naturaldiffusion_amd.synth import synthetic_inception_head
    w, b = synthetic_inception_head(0)
    assert w.dtype == b.dtype == torch.float32 and tuple(w.shape) == (1008, 2048) and tuple(b.shape) == (1008,)
    assert abs(float(w.std()) - 2.0 / math.sqrt(2048)) <= 0.01 * 2.0 / math.sqrt(2048) and abs(float(b.std()) - 0.5) <= 0.05
    w2, b2 = synthetic_inception_head(0)
    assert torch.equal(w, w2) and torch.equal(b, b2) and not torch.equal(w, synthetic_inception_head(1)[0])
    w, b = synthetic_inception_head(3, classes=130, d=64)
    assert tuple(w.shape) == (130, 64) and tuple(b.shape) == (130,)


def test_calc_is_blocked_without_the_weights(tmp_path, monkeypatch):
    from naturaldiffusion_amd import CIFAR10NaturalInference as M
    monkeypatch.setenv("NATINF_INCEPTION_WEIGHTS", str(tmp_path / "absent.pth"))
    imgs = torch.zeros(4, 32, 32, 3, dtype=torch.uint8)
    for fn in (M.calc_is, M.calc_is_sharded):
        with pytest.raises(FileNotFoundError, match="fid: blocked"):
            fn(imgs, "cpu")
    with pytest.raises(FileNotFoundError, match="fid: blocked"):
        M.fid_inception_head("cpu")


def test_the_oracle_against_itself():
    """shifting the bias changes nothing; the planted-class conditions hold at every GPU case's shape"""
    for n, C, d in GPU_CASES:
        cs = IO.case(n, C, d)
        a, W, b = cs["a"], cs["W"], cs["b"]
        B = IO.bounds(a, W, b)
        moved = IO.bounds(a, W, b + 12.0)
        assert float((moved["lse"] - B["lse"] - 12.0).abs().max()) <= 1e-5                     # (the bias is fp32: the shift rounds it)
        shifted = IO.row_stats(IO.logits(a, W, b) + 12.0)
        assert float((shifted["h"] - B["h"]).abs().max()) <= 1e-12 and float((shifted["p"] - B["p"]).abs().max()) <= 1e-12
        assert torch.equal(shifted["top"], B["top"]) and abs(IO.log_score(shifted["p"]) - B["log_is"]) <= 1e-12
        assert len(cs["planted"]) == len([k for k, _ in enumerate(IO.planted_classes(C)) if 5 * k + 3 < n])
        z = IO.logits(a, W, b)
        rows = [r for _, r in cs["planted"]]
        for c, r in cs["planted"]:
            assert int(B["top"][r]) == c and float(B["gap"][r]) >= 100 * float(B["E"][r]), (n, C, d, c, r)
            assert float((IO.lse_without(z, c)[r] - B["lse"][r]).abs()) >= 100 * float(B["lse_bound"][r]), (n, C, d, c, r)
        non = torch.ones(n, dtype=torch.bool)
        non[rows] = False
        assert bool(((IO.lse_with_zero_column(z) - B["lse"]).abs() >= 100 * B["lse_bound"])[non].all()), (n, C, d)
        assert float((B["gap"] >= 100 * B["E"]).double().mean()) >= 0.9, (n, C, d)
        if n > 1:
            assert B["log_is"] >= 100 * B["log_is_bound"], (n, C, d, B["log_is"], B["log_is_bound"])
        else:
            assert abs(B["log_is"]) <= 1e-15                       # one row is its own marginal: IS = 1 whatever the head
    assert IO.planted_classes(1008) == [0, 31, 32, 63, 64, 127, 128, 895, 896, 1006, 1007] and IO.planted_classes(2) == [0, 1]
    assert len(IO.case(130, 1008, 2048)["planted"]) == 11
