"""numpy mirror of k_fold_up_conv (csrc/up_fold.h): the four 2x2 phase kernels of a 3x3 convolution over a 2x nearest-up-sampled image.

Output pixel (2 i + a, 2 j + b) of conv3x3(nearest_up_2x(h), W, padding=1) reads rows i + a - 1 + ty and columns j + b - 1 + tx (ty, tx in {0, 1}) of h itself.
Summation order, the one the device kernel documents: rows first, then columns, each pair as (W[lo] + W[hi])."""
import numpy as np


def fold_up_numpy(w, w_mul=1.0):
    """w [N][C][3][3] -> Wp [a][b][N][C][ty][tx], in w's dtype (float32: the device kernel's arithmetic, bit for bit)"""
    out = np.empty((2, 2) + w.shape[:2] + (2, 2), dtype=w.dtype)
    m = w.dtype.type(w_mul)
    for a in (0, 1):
        rows = [w[:, :, 0, :], w[:, :, 1, :] + w[:, :, 2, :]] if a == 0 else [w[:, :, 0, :] + w[:, :, 1, :], w[:, :, 2, :]]
        for b in (0, 1):
            for ty in (0, 1):
                r = rows[ty]
                cols = [r[..., 0], r[..., 1] + r[..., 2]] if b == 0 else [r[..., 0] + r[..., 1], r[..., 2]]
                for tx in (0, 1):
                    out[a, b, :, :, ty, tx] = cols[tx] * m
    return out
