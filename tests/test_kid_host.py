"""Host side of the Kernel Inception Distance (include/natinf_kid.h; naturaldiffusion_amd/kid.py): every refusal of the two entries, the workspace query,
the block partition and the MMD^2 by hand, the import without the library and the blocked path of the two job functions.  No GPU."""
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

from naturaldiffusion_amd import _lib
from naturaldiffusion_amd import kid as K

EINVAL = -1
L = _lib.lib

# never dereferenced: every call below must be refused before anything is configured or launched
PTR = 0x1000            # 256-byte aligned, non-null


def _sums(rp=PTR, rs=None, n_rows=4, cp=PTR, cs=None, n_cols=8, d=64, self_offset=-1, gamma=1.0 / 64, coef0=1.0, out=PTR, ws=PTR, ws_bytes=1 << 30):
    rs = max(n_rows, 0) * max(d, 0) if rs is None else rs
    cs = max(n_cols, 0) * max(d, 0) if cs is None else cs
    return L.natinf_kid_row_sums(rp, rs, n_rows, cp, cs, n_cols, d, self_offset, gamma, coef0, out, ws, ws_bytes, None)


def test_argument_errors_are_einval():
    for d in (0, 32, 96, -64, 4096 + 64, 65536):
        assert _sums(d=d) == EINVAL and L.natinf_kid_workspace_bytes(4, 8, d) == EINVAL, d
    for n in (0, -1, (1 << 20) + 1):
        assert _sums(n_rows=n) == EINVAL and _sums(n_cols=n) == EINVAL, n
        assert L.natinf_kid_workspace_bytes(n, 8, 64) == EINVAL and L.natinf_kid_workspace_bytes(4, n, 64) == EINVAL, n
    # null and misaligned pointers
    for name in ("rp", "cp", "out", "ws"):
        assert _sums(**{name: None}) == EINVAL, name
    assert _sums(rp=PTR + 8) == EINVAL and _sums(cp=PTR + 8) == EINVAL and _sums(out=PTR + 4) == EINVAL and _sums(ws=PTR + 16) == EINVAL
    # a plane stride holds the operand's rows at least and keeps every plane 16-byte aligned
    assert _sums(rs=4 * 64 - 8) == EINVAL and _sums(cs=8 * 64 - 8) == EINVAL and _sums(rs=0) == EINVAL and _sums(cs=-512) == EINVAL
    for off in (1, 2, 4, 12):
        assert _sums(rs=4 * 64 + off) == EINVAL and _sums(cs=8 * 64 + off) == EINVAL, off
    # gamma and coef0 are finite
    for bad in (math.inf, -math.inf, math.nan):
        assert _sums(gamma=bad) == EINVAL and _sums(coef0=bad) == EINVAL, bad
    # the left-out column must exist for every row, and something must be left
    for so in (-2, 5, 8, 1 << 40):
        assert _sums(self_offset=so) == EINVAL, so
    assert _sums(n_rows=1, n_cols=1, self_offset=0) == EINVAL
    # a short workspace
    need = L.natinf_kid_workspace_bytes(4, 8, 64)
    assert need > 0 and _sums(ws_bytes=need - 1) == EINVAL and _sums(ws_bytes=0) == EINVAL
    need = L.natinf_kid_workspace_bytes(300, 5000, 2048)
    assert _sums(n_rows=300, n_cols=5000, d=2048, ws_bytes=need - 1) == EINVAL


def test_workspace_bytes_is_monotone():
    ns = [1, 2, 63, 64, 65, 1000, 4096, 32768, 32769, 50000, 65536, 1 << 20]
    cols = [1, 8, 100, 128, 129, 1024, 1025, 5000, 65536, 1 << 20]
    b = np.array([[L.natinf_kid_workspace_bytes(n, c, 2048) for c in cols] for n in ns], dtype=np.int64)
    assert (b > 0).all() and (np.diff(b, axis=0) >= 0).all() and (np.diff(b, axis=1) >= 0).all()
    for d0, d1 in ((64, 2048), (2048, 4096)):
        assert L.natinf_kid_workspace_bytes(5000, 5000, d0) <= L.natinf_kid_workspace_bytes(5000, 5000, d1)
    # a few doubles per row: no N^2 term, and nothing that depends on the rows of the call but their number
    assert L.natinf_kid_workspace_bytes(1 << 20, 1 << 20, 4096) <= 64 * 8 * (1 << 20)
    assert L.natinf_kid_workspace_bytes(2000, 5000, 2048) == 2 * L.natinf_kid_workspace_bytes(1000, 5000, 2048)


def test_block_bounds_by_hand():
    br, bg = K.block_bounds(261, 300, 64)
    assert [len(r) for r in br] == [52, 52, 52, 52, 53] and [len(r) for r in bg] == [60] * 5
    assert [r.start for r in br] == [0, 52, 104, 156, 208] and br[-1].stop == 261 and all(r.step == 1 for r in br + bg)
    assert [(r.start, r.stop) for r in bg] == [(0, 60), (60, 120), (120, 180), (180, 240), (240, 300)]
    br, bg = K.block_bounds(257, 130, 1024)                       # a single block: the whole sets
    assert br == [range(257)] and bg == [range(130)]
    br, bg = K.block_bounds(1024, 1024, 1024)
    assert br == [range(1024)] and bg == [range(1024)]
    br, bg = K.block_bounds(1025, 7, 1024)                        # two blocks: 512 + 513 and 3 + 4
    assert [len(r) for r in br] == [512, 513] and [len(r) for r in bg] == [3, 4]
    br, bg = K.block_bounds(10, 11, 4)                            # 3 blocks: 3 3 4 and 3 4 4
    assert [len(r) for r in br] == [3, 3, 4] and [len(r) for r in bg] == [3, 4, 4]
    with pytest.raises(ValueError, match="fewer than 2"):
        K.block_bounds(300, 5, 64)                                # five blocks of one generated row
    with pytest.raises(ValueError, match="fewer than 2"):
        K.block_bounds(3000, 5, 1024)                             # three blocks: 1, 2, 2
    with pytest.raises(ValueError):
        K.block_bounds(1, 50, 64)
    with pytest.raises(ValueError):
        K.block_bounds(50, 50, 1)


def test_mmd2_from_sums_by_hand():
    # three real rows, two generated: 6 ordered real pairs, 2 ordered generated pairs, 6 cross pairs
    assert K.mmd2_from_sums(12.0, 3, 5.0, 2, 9.0) == 12.0 / 6 + 5.0 / 2 - 2 * 9.0 / 6
    assert K.mmd2_from_sums(0.0, 2, 0.0, 2, 0.0) == 0.0
    # the same kernel value everywhere: the estimate vanishes
    m, n, k = 7, 5, 1.25
    assert abs(K.mmd2_from_sums(k * m * (m - 1), m, k * n * (n - 1), n, k * m * n)) <= 1e-15
    for m, n in ((1, 5), (5, 1), (0, 0)):
        with pytest.raises(ValueError):
            K.mmd2_from_sums(1.0, m, 1.0, n, 1.0)


def test_module_imports_without_the_library(repo_root, tmp_path):
    """block_bounds and mmd2_from_sums are host code: the module imports where libnatinf.so cannot be loaded"""
    code = ("import os, sys; os.environ['NATINF_LIB'] = sys.argv[2]; sys.path.insert(0, sys.argv[1])\n"
            "from naturaldiffusion_amd import kid as K\n"
            "assert 'naturaldiffusion_amd._lib' not in sys.modules\n"
            "print([len(r) for r in K.block_bounds(261, 300, 64)[0]], K.mmd2_from_sums(12.0, 3, 5.0, 2, 9.0))\n")
    p = subprocess.run([sys.executable, "-c", code, str(repo_root), str(tmp_path / "absent.so")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip() == "[52, 52, 52, 52, 53] 1.5"


def test_calc_kid_blocked_without_the_reference_features(tmp_path):
    from naturaldiffusion_amd import CIFAR10NaturalInference as M
    imgs = torch.zeros(4, 32, 32, 3, dtype=torch.uint8)
    for fn in (M.calc_kid, M.calc_kid_sharded):
        with pytest.raises(FileNotFoundError, match="kid: blocked"):
            fn(imgs, tmp_path / "cifar10_pool3.npy", "cpu")
        with pytest.raises(FileNotFoundError, match="kid: blocked"):
            fn(imgs, str(tmp_path / "cifar10_pool3.npy"), "cpu", estimator="full")
