"""Nearest neighbours of one feature set in another, distances and indices, on the HIP library's exact distance sweep (include/natinf_nn.h; DESIGN.md
section 4d-nn): which training image is each generated image closest to, and is it a copy?

Row i of ``nearest``'s result holds the k smallest pairs (d2_ij, j) in lexicographic order -- among equal distances the lower column comes first -- of the
distances ``prdc.py``'s metrics are made of.  A row's result depends on that row and the column set only: the rows split freely over calls and ranks.
In pixel space (``pixel_features``: uint8 values 0..255, unscaled) every squared distance is an exact integer.

This module imports without the library (``summary`` and the shape checks of ``pixel_features`` are host code); ``nearest`` needs the GPU."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .prdc import FeatureSet, _check_k, _lib

MAX_D = 4096                 # include/natinf_prdc.h


def nearest(rows: FeatureSet, cols: FeatureSet, k: int = 1, row_range: Optional[range] = None, self_offset: int = -1) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d2 fp64 [n, k], idx int64 [n, k]) on the device: the k nearest columns of ``cols`` for every row of ``rows``, nearest first.  ``row_range`` (a
    contiguous range, default all) selects the rows -- the same bytes as those rows of the whole call.  ``self_offset`` >= 0 leaves column
    ``self_offset + i`` out of row i of the WHOLE set ``rows`` (a set against itself: 0), whatever ``row_range`` selects; -1 leaves nothing out.
    A slot that no column filled (non-finite features) holds d2 = +inf and idx = -1."""
    L = _lib()
    if rows.d != cols.d:
        raise ValueError("neighbours: the two sets differ in feature width")
    r = range(rows.n) if row_range is None else row_range
    if self_offset < -1:
        raise ValueError("neighbours: self_offset must be -1 or a column offset")
    _check_k(k, cols.n, self_offset)
    d2 = torch.empty(len(r), k, dtype=torch.float64, device=cols.device)
    idx = torch.empty(len(r), k, dtype=torch.int32, device=cols.device)
    if len(r) == 0:
        return d2, idx.long()
    pl, nm = rows.rows(r)
    off = self_offset + r.start if self_offset >= 0 else -1
    nbytes = L.lib.natinf_nn_workspace_bytes(len(r), cols.n, cols.d, k)
    L.check(min(nbytes, 0), "natinf_nn_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cols.device)
    with torch.cuda.device(cols.device):
        L.check(L.lib.natinf_nn_nearest(L.ptr(pl), L.ptr(nm), len(r), L.ptr(cols.planes), L.ptr(cols.norms), cols.n, cols.d, k, off,
                                        L.ptr(d2), L.ptr(idx), L.ptr(ws), nbytes, L.stream_ptr()), "natinf_nn_nearest")
    return d2, idx.long()


def pixel_features(images, device=None) -> torch.Tensor:
    """uint8 [n, H, W, 3] images (device or host) -> fp32 [n, 3 H W] on the device, the values 0..255 unscaled: a uint8 value is exact in the first bf16
    plane of a ``FeatureSet``, so every pixel-space squared distance of the sweep is an exact integer.  The feature width 3 H W must be a multiple of
    64 and at most 4,096 (CIFAR10: 3,072)."""
    images = torch.as_tensor(images)
    if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
        raise ValueError(f"neighbours: images must be uint8 [n, H, W, 3], got {images.dtype} {tuple(images.shape)}")
    d = 3 * int(images.shape[1]) * int(images.shape[2])
    if d % 64 or not (64 <= d <= MAX_D):
        raise ValueError(f"neighbours: {tuple(images.shape[1:3])} images have {d} values each; the sweep takes a multiple of 64 up to {MAX_D}")
    dev = torch.device(device) if device is not None else (images.device if images.is_cuda else torch.device("cuda:0"))
    return images.to(dev).reshape(images.shape[0], d).float()


def summary(d2) -> dict:
    """dict(n, min, median, mean, copies) of the NEAREST distance of every row (``d2[:, 0]``; ``d2``: [n, k] or [n], tensor or array): what a report prints
    beside the FID table.  ``copies`` counts the rows whose nearest distance is exactly 0.  Host code."""
    a = np.asarray(d2.detach().cpu() if isinstance(d2, torch.Tensor) else d2, dtype=np.float64)
    if a.ndim == 2:
        a = a[:, 0]
    if a.ndim != 1 or a.size == 0:
        raise ValueError("neighbours: summary needs a non-empty [n, k] or [n] table of distances")
    return dict(n=int(a.size), min=float(a.min()), median=float(np.median(a)), mean=float(a.mean()), copies=int((a == 0).sum()))
