"""Kernel Inception Distance (Binkowski et al. 2018; TF-GAN's ``kernel_classifier_distance``) of a generated feature set against a real one, on the HIP
library (include/natinf_kid.h).

    k(x, y) = (gamma x.y + coef0)^3                    gamma = 1 / d, coef0 = 1 by default
    MMD^2   = sum_{i != j} k(x_i, x_j) / (m (m - 1)) + sum_{i != j} k(y_i, y_j) / (n (n - 1)) - 2 sum_{i, j} k(x_i, y_j) / (m n)        (unbiased; m, n >= 2)

``estimator="full"`` is that expression on the whole sets; ``estimator="blocks"`` is TF-GAN's ``kernel_classifier_distance_and_std_from_activations``: the mean
of the MMD^2 of ``n_blocks`` pairs of contiguous blocks and its standard error.  Everything on the device is a per-row sum of kernel values over a contiguous
column range (``kernel_row_sums``); a row's sum depends on that row and the column range only, so the rows split freely over calls and ranks.  The sums are
reduced on the host with ``math.fsum``, which rounds the exact sum once: the result does not depend on the order of the rows or on who computed them.

This module imports without the library (``block_bounds`` and ``mmd2_from_sums`` are host code); everything else needs the GPU."""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

from .prdc import FeatureSet, row_slice

ESTIMATORS = ("blocks", "full")
LOCAL = object()             # ``group=LOCAL``: this process alone, whatever process group exists (``group=None`` is the default group, as in torch)


def _lib():
    from . import _lib as L
    return L


def block_bounds(m: int, n: int, max_block_size: int = 1024) -> Tuple[List[range], List[range]]:
    """TF-GAN's partition of ``m`` real and ``n`` generated rows into ``n_blocks = ceil(max(m, n) / max_block_size)`` pairs of contiguous blocks in row
    order: of a set of ``size`` rows the first ``n_blocks - p`` blocks hold ``v = size // n_blocks`` rows and the last ``p = size - v * n_blocks`` hold
    ``v + 1``.  A block of fewer than 2 rows is a ``ValueError`` (the unbiased estimate divides by ``rows - 1``).  Host code."""
    m, n, max_block_size = int(m), int(n), int(max_block_size)
    if max_block_size < 2:
        raise ValueError("kid: max_block_size must be at least 2")
    if m < 2 or n < 2:
        raise ValueError(f"kid: the unbiased estimate needs 2 rows of each set at least, got {m} and {n}")
    n_blocks = -(-max(m, n) // max_block_size)

    def cut(size):
        v = size // n_blocks
        p = size - v * n_blocks
        if v < 2:
            raise ValueError(f"kid: {n_blocks} blocks leave a set of {size} rows a block of {v}: fewer than 2")
        ends = [0]
        for b in range(n_blocks):
            ends.append(ends[-1] + v + (b >= n_blocks - p))
        return [range(ends[b], ends[b + 1]) for b in range(n_blocks)]

    return cut(m), cut(n)


def mmd2_from_sums(sxx: float, m: int, syy: float, n: int, sxy: float) -> float:
    """The unbiased MMD^2 from the three kernel sums: ``sxx`` over the ordered pairs i != j of the ``m`` real rows, ``syy`` the same of the ``n`` generated
    rows, ``sxy`` over all m x n pairs.  Host code."""
    m, n = int(m), int(n)
    if m < 2 or n < 2:
        raise ValueError(f"kid: the unbiased estimate needs 2 rows of each set at least, got {m} and {n}")
    return float(sxx) / (m * (m - 1)) + float(syy) / (n * (n - 1)) - 2.0 * float(sxy) / (m * n)


def _range_in(r: Optional[range], n: int, what: str) -> range:
    r = range(n) if r is None else r
    if r.step != 1 or r.start < 0 or r.stop > n:
        raise ValueError(f"kid: a {what} range must be contiguous and inside the set")
    return r


def kernel_row_sums(rows: FeatureSet, r: range, cols: FeatureSet, c: Optional[range] = None, exclude_self: bool = False,
                    gamma: Optional[float] = None, coef0: float = 1.0) -> torch.Tensor:
    """fp64 [len(r)] on the device: for every row of the contiguous range ``r`` of ``rows`` the sum of ``(gamma a.b + coef0)^3`` over the contiguous column
    range ``c`` of ``cols`` (default: all of them).  ``exclude_self`` (``rows is cols``, ``r`` inside ``c``) leaves the row's own column out.  Both ranges are
    read in place.  A row's sum is the same bytes whichever other rows the call holds."""
    L = _lib()
    if rows.d != cols.d:
        raise ValueError("kid: the two sets differ in feature width")
    if rows.device != cols.device:
        raise ValueError("kid: the two sets are on different devices")
    r, c = _range_in(r, rows.n, "row"), _range_in(c, cols.n, "column")
    if len(c) == 0:
        raise ValueError("kid: an empty column range")
    self_offset = -1
    if exclude_self:
        if rows is not cols or (len(r) and not (c.start <= r.start and r.stop <= c.stop)) or len(c) < 2:
            raise ValueError("kid: exclude_self needs rows of the column set itself, inside a column range of 2 at least")
        self_offset = r.start - c.start
    gamma = 1.0 / rows.d if gamma is None else float(gamma)
    coef0 = float(coef0)
    if not (math.isfinite(gamma) and math.isfinite(coef0)):
        raise ValueError("kid: gamma and coef0 must be finite")
    out = torch.empty(len(r), dtype=torch.float64, device=cols.device)
    if len(r) == 0:
        return out
    d = rows.d
    nbytes = L.lib.natinf_kid_workspace_bytes(len(r), len(c), d)
    L.check(min(nbytes, 0), "natinf_kid_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cols.device)
    esize = rows.planes.element_size()
    with torch.cuda.device(cols.device):
        L.check(L.lib.natinf_kid_row_sums(L.ptr(rows.planes) + r.start * d * esize, rows.n * d, len(r),
                                          L.ptr(cols.planes) + c.start * d * esize, cols.n * d, len(c),
                                          d, self_offset, gamma, coef0, L.ptr(out), L.ptr(ws), nbytes, L.stream_ptr()), "natinf_kid_row_sums")
    return out


def _total(v: torch.Tensor) -> float:
    return math.fsum(v.cpu().tolist())


def _group(group):
    import torch.distributed as dist
    on = group is not LOCAL and dist.is_available() and dist.is_initialized()
    return (dist.get_rank(group), dist.get_world_size(group), on) if on else (0, 1, False)


def _all_gather_f64(mine: torch.Tensor, sizes: List[int], group) -> List[torch.Tensor]:
    """every rank's fp64 vector (``sizes[rank]`` values, known to all) on the host, in rank order"""
    import torch.distributed as dist
    host = dist.get_backend(group) != "nccl"
    pad = torch.zeros(max(max(sizes), 1), dtype=torch.float64, device="cpu" if host else mine.device)
    pad[:mine.numel()] = mine
    parts = [torch.empty_like(pad) for _ in sizes]
    dist.all_gather(parts, pad, group=group)
    return [p[:s].cpu() for p, s in zip(parts, sizes)]


def _sliced_totals(jobs, group) -> List[float]:
    """``jobs``: (rows, cols, exclude_self, gamma, coef0) each.  The exactly rounded total of every job's row sums over ALL rows: this rank sweeps its
    ``row_slice`` against the whole column set, the per-row sums are all-gathered and every rank reduces the same vectors."""
    rank, world, on = _group(group)
    mine = [kernel_row_sums(a, row_slice(a.n, rank, world), b, None, ex, gamma, coef0) for a, b, ex, gamma, coef0 in jobs]
    if not on or world == 1:
        return [_total(v) for v in mine]
    sizes = [sum(len(row_slice(j[0].n, r, world)) for j in jobs) for r in range(world)]
    parts = _all_gather_f64(torch.cat(mine), sizes, group)
    totals, offs = [], [0] * world
    for a, *_ in jobs:
        vals = []
        for r in range(world):
            k = len(row_slice(a.n, r, world))
            vals += parts[r][offs[r]:offs[r] + k].tolist()
            offs[r] += k
        totals.append(math.fsum(vals))
    return totals


def real_self_sum(real, gamma: Optional[float] = None, coef0: float = 1.0, group=None) -> float:
    """The real x real term of the full estimator, ``sum_{i != j} k(x_i, x_j)``: fixed for a reference set, so a caller that scores many generated sets
    against it pays for it once and hands it to ``kid(..., estimator="full", real_self_sum=...)`` (with the same ``gamma`` and ``coef0``)."""
    real = real if isinstance(real, FeatureSet) else FeatureSet(real)
    return _sliced_totals([(real, real, True, gamma, coef0)], group)[0]


def kid(real, gen, estimator: str = "blocks", max_block_size: int = 1024, gamma: Optional[float] = None, coef0: float = 1.0,
        real_self_sum: Optional[float] = None, group=None) -> dict:
    """dict(kid, std, n_blocks, estimator) of ``gen`` against ``real`` (FeatureSet or fp32 [n, d] tensors; every rank holds both whole sets).

    ``"full"``: the unbiased MMD^2 of the whole sets; ``std`` is None and ``n_blocks`` 1.  ``real_self_sum`` (``real_self_sum(real, gamma, coef0)``) spares
    the real x real sweep.  ``"blocks"``: ``block_bounds(m, n, max_block_size)`` cuts both sets, ``est_b`` is the unbiased MMD^2 of real block b against
    generated block b, ``kid`` their mean and ``std = sqrt(var / n_blocks)`` with the sample variance ``var`` (0 for a single block).  Like TF-GAN's, the block
    estimate DEPENDS ON THE ROW ORDER of both sets (which rows meet in a block); the full estimate does not.

    In a process group the full estimator has every rank sweep its ``row_slice`` of the three matrices and all-gathers the per-row sums; the block estimator
    gives rank r the blocks b = r (mod world) and all-gathers the estimates.  Every rank returns the same bytes, the same as one rank's.  ``group=LOCAL``
    takes no part in any group: this process measures everything itself."""
    if estimator not in ESTIMATORS:
        raise ValueError(f"kid: estimator must be one of {ESTIMATORS}")
    real = real if isinstance(real, FeatureSet) else FeatureSet(real)
    gen = gen if isinstance(gen, FeatureSet) else FeatureSet(gen, device=real.device)
    if real.d != gen.d:
        raise ValueError("kid: the two sets differ in feature width")
    m, n = real.n, gen.n
    if estimator == "full":
        if m < 2 or n < 2:
            raise ValueError(f"kid: the unbiased estimate needs 2 rows of each set at least, got {m} and {n}")
        jobs = [(gen, gen, True, gamma, coef0), (real, gen, False, gamma, coef0)]
        if real_self_sum is None:
            jobs.append((real, real, True, gamma, coef0))
        t = _sliced_totals(jobs, group)
        sxx = float(real_self_sum) if real_self_sum is not None else t[2]
        return dict(kid=mmd2_from_sums(sxx, m, t[0], n, t[1]), std=None, n_blocks=1, estimator="full")
    if real_self_sum is not None:
        raise ValueError("kid: real_self_sum belongs to the full estimator")
    br, bg = block_bounds(m, n, max_block_size)
    n_blocks = len(br)
    rank, world, on = _group(group)
    owned = list(range(rank, n_blocks, world))
    # A block's sweep is 16 x 8 thread blocks at 1,024 rows, half of the chip: the three sweeps of a block run beside each other on three streams, and
    # every sweep of every owned block is enqueued before the host waits for the first.  (A sweep's result does not depend on what runs beside it.)
    sums = []
    if owned:
        main = torch.cuda.current_stream(real.device)
        lanes = [torch.cuda.Stream(real.device) for _ in range(3)]
        for lane in lanes:
            lane.wait_stream(main)                              # the planes were written on the caller's stream
        for b in owned:
            for lane, (a, ra, c, rc, own) in zip(lanes, ((real, br[b], real, br[b], True), (gen, bg[b], gen, bg[b], True), (real, br[b], gen, bg[b], False))):
                with torch.cuda.stream(lane):
                    sums.append(kernel_row_sums(a, ra, c, rc, own, gamma, coef0))
        for lane in lanes:
            main.wait_stream(lane)
        for v in sums:
            v.record_stream(main)                               # allocated on a lane, read by the caller's stream below
    flat = torch.cat(sums).cpu().tolist() if sums else []
    est, at = [], 0
    for b in owned:
        tot = []
        for k in (len(br[b]), len(bg[b]), len(br[b])):
            tot.append(math.fsum(flat[at:at + k]))
            at += k
        est.append(mmd2_from_sums(tot[0], len(br[b]), tot[1], len(bg[b]), tot[2]))
    if on and world > 1:
        sizes = [len(range(r, n_blocks, world)) for r in range(world)]
        parts = _all_gather_f64(torch.tensor(est, dtype=torch.float64, device=real.device), sizes, group)
        est = [float(parts[b % world][b // world]) for b in range(n_blocks)]
    mean = math.fsum(est) / n_blocks
    var = math.fsum((e - mean) ** 2 for e in est) / (n_blocks - 1) if n_blocks > 1 else 0.0
    return dict(kid=mean, std=math.sqrt(var / n_blocks), n_blocks=n_blocks, estimator="blocks")
