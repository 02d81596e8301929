"""Improved precision and recall (Kynkaanniemi et al. 2019, the ADM evaluator's definition) and density and coverage (Naeem et al. 2020)
of a generated feature set against a real one, on the HIP library (include/natinf_prdc.h).

With ``r2(S)[j]`` the squared distance from ``S[j]`` to its k-th nearest neighbour in ``S`` (itself left out):

    precision = mean_i [ gen_i  lies in the ball of some real_j ]          density  = mean_i #{ j : gen_i in ball(real_j) } / k
    recall    = mean_i [ real_i lies in the ball of some gen_j  ]          coverage = mean_i [ some gen_j lies in ball(real_i) ]

Every one of them is a mean over ROWS of a count over a whole column set, and a row's count depends on that row and the column set only: the rows
split freely over calls and ranks (``row_slice``), the integer sums are the same bytes for any split.  The N x N distances are never stored.

This module imports without the library (``prdc_from_counts`` and ``row_slice`` are host code); everything else needs the GPU."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

MAX_K = 8                    # include/natinf_prdc.h


def row_slice(n: int, rank: int, world: int) -> range:
    """The contiguous rows of an ``n``-row set that rank ``rank`` of ``world`` measures: every row exactly once over the ranks, sizes differing by
    one at the most (empty when ``n < world`` leaves none)."""
    if not (0 <= rank < world):
        raise ValueError("rank out of range")
    return range(rank * n // world, (rank + 1) * n // world)


def _lib():
    from . import _lib as L
    return L


class FeatureSet:
    """An fp32 ``[n, d]`` feature tensor prepared for the distance kernels: three bf16 planes with hi + mid + lo == feats exactly and the fp64 row
    norms, on the device (``feats`` itself is not kept)."""

    def __init__(self, feats, device=None):
        L = _lib()
        feats = torch.as_tensor(feats)
        if feats.dim() != 2 or feats.dtype != torch.float32:
            raise ValueError(f"prdc: features must be an fp32 [n, d] tensor, got {feats.dtype} {tuple(feats.shape)}")
        dev = torch.device(device) if device is not None else (feats.device if feats.is_cuda else torch.device("cuda:0"))
        feats = feats.to(dev).contiguous()
        self.n, self.d = int(feats.shape[0]), int(feats.shape[1])
        self.device = dev
        self.planes = torch.empty(3, self.n, self.d, dtype=torch.bfloat16, device=dev)
        self.norms = torch.empty(self.n, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib.natinf_prdc_planes(L.ptr(feats), self.n, self.d, L.ptr(self.planes), L.ptr(self.norms), L.stream_ptr()), "natinf_prdc_planes")

    def rows(self, r: range) -> Tuple[torch.Tensor, torch.Tensor]:
        """(planes [3, len(r), d], norms) of a contiguous row range, in the layout the kernels read"""
        if r.step != 1 or r.start < 0 or r.stop > self.n:
            raise ValueError("prdc: a row range must be contiguous and inside the set")
        if len(r) == self.n:
            return self.planes, self.norms
        return self.planes[:, r.start:r.stop].contiguous(), self.norms[r.start:r.stop]


def _check_k(k: int, n_cols: int, self_offset: int) -> None:
    if not (1 <= k <= MAX_K):
        raise ValueError(f"prdc: k must be in 1..{MAX_K}")
    if k + (self_offset >= 0) > n_cols:
        raise ValueError(f"prdc: {n_cols} columns are too few for k = {k}")


def _knn(rows: FeatureSet, r: range, cols: FeatureSet, k: int, self_offset: int) -> torch.Tensor:
    L = _lib()
    if rows.d != cols.d:
        raise ValueError("prdc: the two sets differ in feature width")
    _check_k(k, cols.n, self_offset)
    out = torch.empty(len(r), dtype=torch.float64, device=cols.device)
    if len(r) == 0:
        return out
    pl, nm = rows.rows(r)
    nbytes = L.lib.natinf_prdc_workspace_bytes(len(r), cols.n, cols.d, k)
    L.check(min(nbytes, 0), "natinf_prdc_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cols.device)
    with torch.cuda.device(cols.device):
        L.check(L.lib.natinf_prdc_knn_radius(L.ptr(pl), L.ptr(nm), len(r), L.ptr(cols.planes), L.ptr(cols.norms), cols.n, cols.d, k, self_offset,
                                             L.ptr(out), L.ptr(ws), nbytes, L.stream_ptr()), "natinf_prdc_knn_radius")
    return out


def _balls(rows: FeatureSet, r: range, cols: FeatureSet, r2_rows: Optional[torch.Tensor], r2_cols: Optional[torch.Tensor], self_offset: int = -1):
    """(cnt_row_ball, cnt_col_ball): int32 [len(r)] each, None where its radii are None"""
    L = _lib()
    if rows.d != cols.d:
        raise ValueError("prdc: the two sets differ in feature width")
    mk = lambda on: torch.empty(len(r), dtype=torch.int32, device=cols.device) if on else None
    cr, cc = mk(r2_rows is not None), mk(r2_cols is not None)
    if len(r) == 0:
        return cr, cc
    pl, nm = rows.rows(r)
    with torch.cuda.device(cols.device):
        L.check(L.lib.natinf_prdc_ball_counts(L.ptr(pl), L.ptr(nm), len(r), L.ptr(cols.planes), L.ptr(cols.norms), cols.n, cols.d, self_offset,
                                              L.ptr(r2_rows), L.ptr(r2_cols), L.ptr(cr), L.ptr(cc), L.stream_ptr()), "natinf_prdc_ball_counts")
    return cr, cc


def _check_radii(r2: torch.Tensor, a: FeatureSet, name: str) -> torch.Tensor:
    if r2.dtype != torch.float64 or tuple(r2.shape) != (a.n,) or r2.device != a.norms.device:
        raise ValueError(f"prdc: {name} must be fp64 [{a.n}] on {a.norms.device}, the radii of the whole set")
    return r2.contiguous()


def knn_radii(a: FeatureSet, k: int, rows: Optional[range] = None) -> torch.Tensor:
    """fp64 [len(rows)] on the device: the squared distance from row i of ``a`` to its k-th nearest neighbour in ``a``, itself left out; ``rows`` (a
    contiguous range, default all) selects the rows -- the same bytes as those rows of the whole call."""
    r = range(a.n) if rows is None else rows
    return _knn(a, r, a, k, r.start)


def prdc_counts(real: FeatureSet, gen: FeatureSet, k: int, rows_real: Optional[range] = None, rows_gen: Optional[range] = None,
                r2_real: Optional[torch.Tensor] = None, r2_gen: Optional[torch.Tensor] = None) -> dict:
    """The four per-row count vectors (int32, on the device) for the given row ranges (default all rows):

        gen_in_real_balls  [rows_gen]   #{ j : gen_i in ball(real_j) }      -> precision, density
        real_in_gen_balls  [rows_real]  #{ j : real_i in ball(gen_j) }      -> recall
        gen_in_own_ball    [rows_real]  #{ j : gen_j in ball(real_i) }      -> coverage
        real_rows, gen_rows             how many rows each covers

    The radii are those of the WHOLE sets (every rank computes them all: 2 of the 4 distance passes at world 1, and the part that does not shrink with the world).
    A caller that splits the rows over several calls passes ``r2_real`` / ``r2_gen`` (``knn_radii(real, k)``, ``knn_radii(gen, k)``: fp64 [n] on the device) and
    pays for them once; they come back in the result under the same names."""
    if real.d != gen.d:
        raise ValueError("prdc: the two sets differ in feature width")
    rr = range(real.n) if rows_real is None else rows_real
    rg = range(gen.n) if rows_gen is None else rows_gen
    r2_real = knn_radii(real, k) if r2_real is None else _check_radii(r2_real, real, "r2_real")
    r2_gen = knn_radii(gen, k) if r2_gen is None else _check_radii(r2_gen, gen, "r2_gen")
    _, gen_in_real = _balls(gen, rg, real, None, r2_real)
    own, real_in_gen = _balls(real, rr, gen, r2_real[rr.start:rr.stop], r2_gen)
    return dict(gen_in_real_balls=gen_in_real, real_in_gen_balls=real_in_gen, gen_in_own_ball=own, real_rows=len(rr), gen_rows=len(rg),
                r2_real=r2_real, r2_gen=r2_gen)


def count_sums(counts: dict) -> np.ndarray:
    """int64 [6]: what crosses ranks -- (rows of gen in some real ball, sum of gen's counts, gen rows, real rows in some gen ball, real rows whose ball holds
    a gen sample, real rows)"""
    g, r, o = counts["gen_in_real_balls"], counts["real_in_gen_balls"], counts["gen_in_own_ball"]
    return np.array([int((g > 0).sum()), int(g.sum(dtype=torch.int64)), counts["gen_rows"], int((r > 0).sum()), int((o > 0).sum()), counts["real_rows"]],
                    dtype=np.int64)


def prdc_from_sums(sums, k: int) -> dict:
    s = [int(v) for v in sums]
    if s[2] <= 0 or s[5] <= 0:
        raise ValueError("prdc: an empty set")
    return dict(precision=s[0] / s[2], recall=s[3] / s[5], density=s[1] / (k * s[2]), coverage=s[4] / s[5])


def prdc_from_counts(gen_in_real_balls, real_in_gen_balls, gen_in_own_ball, k: int) -> dict:
    """dict(precision, recall, density, coverage) from the per-row counts of the WHOLE sets (arrays or tensors of integers).  Host code."""
    g, r, o = (np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v).astype(np.int64) for v in (gen_in_real_balls, real_in_gen_balls, gen_in_own_ball))
    if r.shape != o.shape:
        raise ValueError("prdc: the two count vectors of the real rows differ in length")
    return prdc_from_sums([(g > 0).sum(), g.sum(), g.size, (r > 0).sum(), (o > 0).sum(), r.size], k)


def prdc(real, gen, k: int = 3, group=None) -> dict:
    """dict(precision, recall, density, coverage) of ``gen`` against ``real`` (FeatureSet or fp32 [n, 2048]-style tensors; every rank holds both whole sets).
    In a process group each rank measures ``row_slice`` of both sets against the whole sets, the six integer sums are combined with one all-reduce and every rank
    returns the same four numbers -- the same as one rank's."""
    import torch.distributed as dist
    real = real if isinstance(real, FeatureSet) else FeatureSet(real)
    gen = gen if isinstance(gen, FeatureSet) else FeatureSet(gen, device=real.device)
    on = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(group), dist.get_world_size(group)) if on else (0, 1)
    sums = count_sums(prdc_counts(real, gen, k, row_slice(real.n, rank, world), row_slice(gen.n, rank, world)))
    if on:
        t = torch.from_numpy(sums)
        t = t.to(real.device) if dist.get_backend(group) == "nccl" else t
        dist.all_reduce(t, group=group)
        sums = t.cpu().numpy()
    return prdc_from_sums(sums, k)


def debug_dist2(rows: FeatureSet, cols: FeatureSet, self_offset: int = -1) -> torch.Tensor:
    """fp64 [rows.n, cols.n] by the kernels' own tile arithmetic (test hook; at most 2^20 entries)"""
    L = _lib()
    out = torch.empty(rows.n, cols.n, dtype=torch.float64, device=cols.device)
    with torch.cuda.device(cols.device):
        L.check(L.lib.natinf_prdc_debug_dist2(L.ptr(rows.planes), L.ptr(rows.norms), rows.n, L.ptr(cols.planes), L.ptr(cols.norms), cols.n, cols.d, self_offset,
                                              L.ptr(out), L.stream_ptr()), "natinf_prdc_debug_dist2")
    return out
