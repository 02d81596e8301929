"""Inception Score (Salimans et al. 2016; TF-GAN's ``classifier_score_from_logits``) of a feature set under a classifier head, on the HIP library
(include/natinf_is.h).  It needs no reference set.

    z_i     = W a_i + b                                  the logits of row i (the distance kernels' dot products, then fp64)
    p_i     = softmax(z_i),   h_i = sum_j p_ij log p_ij
    pbar    = mean_i p_i                                 kept as integers: Q_j = sum_i llrint(2^42 p_ij), pbar_j = Q_j / (n 2^42)
    log IS  = mean_i h_i - sum_j pbar_j log pbar_j       = mean_i KL(p_i || pbar)
    IS      = exp(log IS)

Everything on the device is a function of one row and the head (``row_stats``), except the class sums, which are integers: both split freely over calls
and ranks.  The host reduces the ``h_i`` with ``math.fsum``, which rounds the exact sum once, and the class sums as Python ints: the score does not depend
on the order of the rows or on who computed them.

This module imports without the library (``split_bounds`` and ``log_score`` are host code); everything else needs the GPU."""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

from .kid import LOCAL, _all_gather_f64, _group
from .prdc import FeatureSet

FRAC_BITS = 42               # include/natinf_is.h
MAX_ROWS = 1 << 20           # rows one call, and one vector of class sums, takes
MAX_CLASSES = 4096


def _lib():
    from . import _lib as L
    return L


class ClassifierHead:
    """A linear classifier on the features: fp32 weights ``[C, d]`` prepared as the head rows' planes (a ``FeatureSet``) and the fp32 bias ``[C]`` (or None)
    on the device."""

    def __init__(self, weight, bias=None, device=None):
        weight = torch.as_tensor(weight)
        if weight.dim() != 2 or weight.dtype != torch.float32:
            raise ValueError(f"iscore: the head's weights must be an fp32 [classes, d] tensor, got {weight.dtype} {tuple(weight.shape)}")
        if not (1 <= weight.shape[0] <= MAX_CLASSES):
            raise ValueError(f"iscore: 1 to {MAX_CLASSES} classes, got {weight.shape[0]}")
        if bias is not None:
            bias = torch.as_tensor(bias)
            if bias.dtype != torch.float32 or tuple(bias.shape) != (weight.shape[0],):
                raise ValueError(f"iscore: the bias must be fp32 [{weight.shape[0]}], got {bias.dtype} {tuple(bias.shape)}")
        self.rows = FeatureSet(weight, device=device)
        self.classes, self.d, self.device = self.rows.n, self.rows.d, self.rows.device
        self.bias = None if bias is None else bias.to(self.device).contiguous()

    def without_bias(self) -> "ClassifierHead":
        """this head on the same planes, scoring W a alone"""
        import copy
        plain = copy.copy(self)
        plain.bias = None
        return plain


def row_stats(feats: FeatureSet, r: Optional[range], head: ClassifierHead) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(neg_entropy fp64 [len(r)], lse fp64 [len(r)], top int32 [len(r)], class_sums int64 [C]) on the device for the contiguous row range ``r`` of ``feats``
    (default: all rows), read in place: ``h_i = sum_j p_ij log p_ij``, the log-sum-exp of the row's logits, its first largest class, and
    ``Q_j = sum_i llrint(2^42 p_ij)`` over exactly those rows.  A row's three values are the same bytes whichever other rows the call holds; the class sums of
    the parts of any split add up to the whole call's integers."""
    L = _lib()
    if feats.d != head.d:
        raise ValueError("iscore: the features and the head differ in feature width")
    if feats.device != head.device:
        raise ValueError("iscore: the features and the head are on different devices")
    r = range(feats.n) if r is None else r
    if r.step != 1 or r.start < 0 or r.stop > feats.n:
        raise ValueError("iscore: a row range must be contiguous and inside the set")
    n = len(r)
    if n > MAX_ROWS:
        raise ValueError(f"iscore: at most {MAX_ROWS} rows in one call, got {n}")
    dev = head.device
    h = torch.empty(n, dtype=torch.float64, device=dev)
    lse = torch.empty(n, dtype=torch.float64, device=dev)
    top = torch.empty(n, dtype=torch.int32, device=dev)
    sums = torch.zeros(head.classes, dtype=torch.int64, device=dev)
    if n == 0:
        return h, lse, top, sums
    d = feats.d
    nbytes = L.lib.natinf_is_workspace_bytes(n, head.classes, d)
    L.check(min(nbytes, 0), "natinf_is_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    esize = feats.planes.element_size()
    with torch.cuda.device(dev):
        L.check(L.lib.natinf_is_row_stats(L.ptr(feats.planes) + r.start * d * esize, feats.n * d, n, L.ptr(head.rows.planes), head.classes * d, head.classes, d,
                                          L.ptr(head.bias), L.ptr(h), L.ptr(lse), L.ptr(top), L.ptr(sums), L.ptr(ws), nbytes, L.stream_ptr()),
                "natinf_is_row_stats")
    return h, lse, top, sums


def split_bounds(n: int, splits: int) -> List[range]:
    """Split k of ``n`` rows in order is ``range(k * n // splits, (k + 1) * n // splits)``.  A split of 0 rows is a ``ValueError``.  Host code."""
    n, splits = int(n), int(splits)
    if splits < 1:
        raise ValueError("iscore: splits must be at least 1")
    if n < splits:
        raise ValueError(f"iscore: {splits} splits leave a set of {n} rows a split of 0 rows")
    return [range(k * n // splits, (k + 1) * n // splits) for k in range(splits)]


def log_score(neg_entropy_values, class_sums, n: int) -> float:
    """log IS of ``n`` rows from their ``h_i`` (any order) and the class sums ``Q_j`` of exactly those rows: ``fsum(h) / n - fsum(pbar_j log pbar_j)`` over the
    classes with ``Q_j > 0``, ``pbar_j = Q_j / (n 2^42)`` (a quotient of Python ints: rounded once).  Host code."""
    n = int(n)
    h = neg_entropy_values.cpu().tolist() if isinstance(neg_entropy_values, torch.Tensor) else [float(v) for v in neg_entropy_values]
    q = class_sums.cpu().tolist() if isinstance(class_sums, torch.Tensor) else [int(v) for v in class_sums]
    if n < 1 or len(h) != n:
        raise ValueError(f"iscore: {len(h)} row values for n = {n}")
    if min(q) < 0:
        raise ValueError("iscore: a negative class sum")
    den = n << FRAC_BITS
    terms = []
    for v in q:
        if v > 0:
            pbar = int(v) / den
            terms.append(pbar * math.log(pbar))
    return math.fsum(h) / n - math.fsum(terms)


def _summary(log_is: List[float], n: int) -> dict:
    scores = [math.exp(v) for v in log_is]
    k = len(scores)
    mean = math.fsum(scores) / k
    std = math.sqrt(math.fsum((s - mean) ** 2 for s in scores) / k) if k > 1 else None
    return dict(**{"is": mean}, std=std, log_is=log_is, splits=k, n=n)


def inception_score(feats, head: ClassifierHead, splits: int = 1, group=None) -> dict:
    """dict(is, std, log_is, splits, n) of ``feats`` (a ``FeatureSet`` or an fp32 [n, d] tensor) under ``head``: ``log_is[k]`` is the log score of split k of
    ``split_bounds(n, splits)``, ``is`` the mean of the splits' scores ``exp(log_is[k])`` and ``std`` their population standard deviation (the usual
    protocol; None for one split).  ``splits=10`` is the protocol of Salimans et al.; like theirs, a split's score depends on which rows it holds.

    In a process group every rank passes ITS rows only and no feature is gathered: the global order is rank 0's rows, then rank 1's, ... (the order
    ``calc_kid_sharded`` gathers in); the ranks all-gather their counts, each runs ``row_stats`` on the intersection of its rows with every split, the
    ``[splits, C]`` integer class sums are all-reduced and the ``h_i`` all-gathered.  Every rank returns the same bytes: those one process returns on the
    gathered order.  ``group=LOCAL`` takes no part in any group: this process scores its own rows."""
    feats = feats if isinstance(feats, FeatureSet) else FeatureSet(feats, device=head.device)
    rank, world, on = _group(group)
    on = on and world > 1
    counts = [feats.n]
    if on:
        import torch.distributed as dist
        host = dist.get_backend(group) != "nccl"
        mine = torch.tensor([feats.n], dtype=torch.int64, device="cpu" if host else head.device)
        parts = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine, group=group)
        counts = [int(p) for p in parts]
    n = sum(counts)
    bounds = split_bounds(n, splits)
    first = sum(counts[:rank]) if on else 0                         # the global index of this rank's row 0
    hs, sums = [], []
    for b in bounds:
        lo = min(max(b.start, first), first + feats.n)
        hi = max(lo, min(b.stop, first + feats.n))
        h, _, _, q = row_stats(feats, range(lo - first, hi - first), head)
        hs.append(h)
        sums.append(q)
    h_mine, q_all = torch.cat(hs), torch.stack(sums)               # the splits are contiguous and ascending: h_mine is this rank's rows in order
    if on:
        q_all = q_all.cpu() if host else q_all
        dist.all_reduce(q_all, group=group)
        h_all = torch.cat(_all_gather_f64(h_mine, counts, group))
    else:
        h_all = h_mine.cpu()
    q_all = q_all.cpu()
    return _summary([log_score(h_all[b.start:b.stop], q_all[k], len(b)) for k, b in enumerate(bounds)], n)
