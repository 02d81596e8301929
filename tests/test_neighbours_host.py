"""Host side of the nearest-neighbour search (include/natinf_nn.h; naturaldiffusion_amd/neighbours.py): the workspace query, every refusal of
natinf_nn_nearest with no device present, pixel_features' shape checks, summary on a hand-made table and the neighbour sheet's layout.  No GPU."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from naturaldiffusion_amd import _lib
from naturaldiffusion_amd import neighbours as N

EINVAL = -1
L = _lib.lib

# never dereferenced: every call below must be refused before anything is configured or launched
PTR = 0x1000            # 256-byte aligned, non-null


def _nn(rp=PTR, rn=PTR, n_rows=4, cp=PTR, cn=PTR, n_cols=8, d=64, k=3, self_offset=-1, d2=PTR, idx=PTR, ws=PTR, ws_bytes=1 << 30):
    return L.natinf_nn_nearest(rp, rn, n_rows, cp, cn, n_cols, d, k, self_offset, d2, idx, ws, ws_bytes, None)


def test_workspace_bytes_is_monotone_and_negative_outside_the_limits():
    ns = [1, 2, 63, 64, 65, 1000, 4096, 32768, 32769, 50000, 65536, 1 << 20]
    cols = [8, 100, 129, 5000, 65536, 1 << 20]
    b = np.array([[L.natinf_nn_workspace_bytes(n, c, 3072, 3) for c in cols] for n in ns], dtype=np.int64)
    assert (b > 0).all() and (np.diff(b, axis=0) >= 0).all() and (np.diff(b, axis=1) >= 0).all()
    for d0, d1 in ((64, 2048), (2048, 4096)):
        for k0, k1 in ((1, 3), (3, 8)):
            assert L.natinf_nn_workspace_bytes(5000, 5000, d0, k0) <= L.natinf_nn_workspace_bytes(5000, 5000, d1, k1)
    # distances and indices of the column ranges' lists: linear in n_rows, no N^2 term
    assert L.natinf_nn_workspace_bytes(1 << 20, 1 << 20, 4096, 8) <= 1024 * (1 << 20)
    assert L.natinf_nn_workspace_bytes(50000, 50000, 3072, 8) < 1 << 28          # the 50,000 x 50,000 fp32 matrix is 10 GB
    for d in (0, 32, 96, -64, 4096 + 64):
        assert L.natinf_nn_workspace_bytes(4, 8, d, 3) == EINVAL, d
    for n in (0, -1, (1 << 20) + 1):
        assert L.natinf_nn_workspace_bytes(n, 8, 64, 3) == EINVAL and L.natinf_nn_workspace_bytes(4, n, 64, 3) == EINVAL, n
    for k in (0, -1, 9):
        assert L.natinf_nn_workspace_bytes(4, 8, 64, k) == EINVAL, k
    assert L.natinf_nn_workspace_bytes(4, 3, 64, 4) == EINVAL and L.natinf_nn_workspace_bytes(4, 4, 64, 4) > 0


def test_argument_errors_are_einval_without_a_device():
    for d in (0, 32, 96, -64, 4096 + 64, 65536):
        assert _nn(d=d) == EINVAL, d
    for n in (0, -1, (1 << 20) + 1):
        assert _nn(n_rows=n) == EINVAL and _nn(n_cols=n) == EINVAL, n
    for k in (0, -1, 9):
        assert _nn(k=k) == EINVAL, k
    # k + (self_offset >= 0) <= n_cols
    assert _nn(n_cols=3, k=4) == EINVAL
    assert _nn(n_rows=2, n_cols=3, k=3, self_offset=0) == EINVAL
    assert _nn(n_rows=1, n_cols=8, k=8, self_offset=0) == EINVAL
    # the left-out column must exist for every row
    for so in (-2, 5, 8, 1 << 40):
        assert _nn(self_offset=so) == EINVAL, so
    # null and misaligned pointers: planes 16 bytes, norms and distances 8, indices 4, workspace 256
    for name in ("rp", "rn", "cp", "cn", "d2", "idx", "ws"):
        assert _nn(**{name: None}) == EINVAL, name
    assert _nn(rp=PTR + 8) == EINVAL and _nn(cp=PTR + 8) == EINVAL and _nn(rn=PTR + 4) == EINVAL and _nn(cn=PTR + 4) == EINVAL
    assert _nn(d2=PTR + 4) == EINVAL and _nn(idx=PTR + 2) == EINVAL and _nn(ws=PTR + 16) == EINVAL and _nn(ws=PTR + 128) == EINVAL
    need = L.natinf_nn_workspace_bytes(4, 8, 64, 3)
    assert need > 0 and _nn(ws_bytes=need - 1) == EINVAL and _nn(ws_bytes=0) == EINVAL and _nn(ws_bytes=-1) == EINVAL


def test_pixel_features_refuses_bad_shapes():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    for bad in (u8(2, 32, 32), u8(2, 32, 32, 1), u8(2, 3, 32, 32), u8(2, 5, 5, 3), u8(2, 2, 2, 3), u8(2, 64, 32, 3), u8(0, 7, 3, 3)):
        with pytest.raises(ValueError, match="neighbours"):
            N.pixel_features(bad)
    with pytest.raises(ValueError, match="uint8"):
        N.pixel_features(torch.zeros(2, 32, 32, 3))
    with pytest.raises(ValueError, match="uint8"):
        N.pixel_features(np.zeros((2, 32, 32, 3), np.int16))
    x = torch.arange(2 * 8 * 8 * 3, dtype=torch.int64).remainder(256).to(torch.uint8).reshape(2, 8, 8, 3)        # 192 values an image
    f = N.pixel_features(x, device="cpu")
    assert f.dtype == torch.float32 and tuple(f.shape) == (2, 192) and torch.equal(f, x.reshape(2, 192).float()) and float(f.max()) == 255.0
    assert torch.equal(N.pixel_features(x.numpy(), device="cpu"), f)


def test_summary_by_hand():
    d2 = np.array([[4.0, 9.0], [0.0, 1.0], [1.0, 1.0], [0.0, 0.0], [10.0, 12.0]])
    want = dict(n=5, min=0.0, median=1.0, mean=3.0, copies=2)
    assert N.summary(d2) == want and N.summary(torch.tensor(d2)) == want and N.summary(d2[:, 0]) == want
    assert N.summary(np.array([[2.5]])) == dict(n=1, min=2.5, median=2.5, mean=2.5, copies=0)
    assert N.summary(np.array([1.0, 3.0]))["median"] == 2.0
    inf = N.summary(np.array([[np.inf], [0.0]]))
    assert inf["copies"] == 1 and inf["min"] == 0.0 and inf["mean"] == np.inf
    assert all(type(v) in (int, float) for v in N.summary(d2).values())                        # plain host numbers: a report prints them
    for bad in (np.zeros((0, 3)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            N.summary(bad)


def test_module_imports_without_the_library(repo_root, tmp_path):
    """summary and pixel_features' checks are host code: the module imports where libnatinf.so cannot be loaded"""
    code = ("import os, sys; os.environ['NATINF_LIB'] = sys.argv[2]; sys.path.insert(0, sys.argv[1])\n"
            "from naturaldiffusion_amd import neighbours as N\n"
            "assert 'naturaldiffusion_amd._lib' not in sys.modules\n"
            "print(N.summary([[0.0, 1.0], [4.0, 5.0]])['copies'])\n")
    p = subprocess.run([sys.executable, "-c", code, str(repo_root), str(tmp_path / "absent.so")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.split() == ["1"]


def test_neighbour_sheet_layout(tmp_path):
    """each image followed by its neighbours, 2 pixels of padding: read back with an independent PNG decoder"""
    from PIL import Image
    from naturaldiffusion_amd import CIFAR10NaturalInference as M
    g = torch.Generator().manual_seed(1)
    imgs = torch.randint(1, 256, (5, 8, 8, 3), generator=g, dtype=torch.uint8)
    ref = torch.randint(1, 256, (7, 8, 8, 3), generator=g, dtype=torch.uint8)
    idx = np.array([[3, 0], [6, 6], [1, -1], [0, 2], [5, 4]])
    M.save_neighbour_sheet(imgs, ref, idx, tmp_path / "sheet.png", count=3)
    got = np.asarray(Image.open(tmp_path / "sheet.png"))
    assert got.shape == (2 + 3 * 10, 2 + 3 * 10, 3)
    tile = lambda i, t: got[2 + 10 * i:10 + 10 * i, 2 + 10 * t:10 + 10 * t]
    for i in range(3):
        assert np.array_equal(tile(i, 0), imgs[i].numpy())
        for t in range(2):
            assert np.array_equal(tile(i, t + 1), ref[idx[i, t]].numpy() if idx[i, t] >= 0 else np.zeros((8, 8, 3), np.uint8))
    mask = np.ones(got.shape[:2], bool)
    for i in range(3):
        for t in range(3):
            mask[2 + 10 * i:10 + 10 * i, 2 + 10 * t:10 + 10 * t] = False
    assert not got[mask].any()
    M.save_neighbour_sheet(imgs, ref, idx, tmp_path / "all.png", count=99)                   # no more lines than images
    assert np.asarray(Image.open(tmp_path / "all.png")).shape == (2 + 5 * 10, 32, 3)
    with pytest.raises(ValueError, match="outside"):
        M.save_neighbour_sheet(imgs, ref, idx + 3, tmp_path / "bad.png")
    with pytest.raises(ValueError, match="sheet"):
        M.save_neighbour_sheet(imgs, ref, idx[:4], tmp_path / "bad.png")
