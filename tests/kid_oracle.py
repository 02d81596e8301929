"""fp64 definition of the Kernel Inception Distance (include/natinf_kid.h; naturaldiffusion_amd/kid.py) in plain torch, and the bound on what the device
may differ from it by.  Inputs are prdc_oracle.cluster_feats.

The bound is derived, not measured from the code under test.  The dot product s_ij is the distance kernels' own, whose measured band is
BAND = 2^-21 of |a|^2 + |b|^2 on d2 = |a|^2 + |b|^2 - 2 s (tests/test_gpu_prdc.py): s moves by half of it,

    e_ij = 2^-22 (|a_i|^2 + |b_j|^2).

With u = gamma s + coef0 and |du| <= |gamma| e, the mean value theorem on u^3 gives |dk| <= 3 (|u| + |gamma| e)^2 |gamma| e.  Everything after s is fp64:
three roundings of 2^-53 on k and, in a row's sum, chains of at most n / 64 + 16 additions (2^-39 of the sum of |k| at n = 2^20 in the worst case, its
square root typically); the term 1e-12 |u|^3 stands for those, beside a first term that is 1e-6 |k| on these inputs:

    dk_ij         <= 3 (|u_ij| + |gamma| e_ij)^2 |gamma| e_ij + 1e-12 |u_ij|^3
    bound(row i)   = sum_j dk_ij                                  (the left-out column left out)
    bound(MMD^2)   = the three normalised sums of dk with all signs positive
    bound(mean of block estimates) = the mean of the blocks' bounds
    bound(std)     = |bounds|_2 / sqrt(B (B - 1)): std = |est - mean|_2 / sqrt(B (B - 1)), centring is a projection (it lengthens no vector), and the norm
                     of a vector moves by no more than the norm of what is added to it."""
import math

import torch

E_REL = 2.0 ** -22           # half of tests/test_gpu_prdc.py's BAND


def _gamma(a, gamma):
    return 1.0 / a.shape[1] if gamma is None else float(gamma)


def kernel_matrix(a, b, gamma=None, coef0=1.0):
    """fp64 [na, nb]: (gamma a.b + coef0)^3"""
    u = _gamma(a, gamma) * (a.double() @ b.double().t()) + coef0
    return u * u * u


def delta_k(a, b, gamma=None, coef0=1.0):
    """fp64 [na, nb]: the bound on |k_device - k_fp64| of every entry"""
    g = abs(_gamma(a, gamma))
    a, b = a.double(), b.double()
    u = (_gamma(a, gamma) * (a @ b.t()) + coef0).abs()
    e = E_REL * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :])
    return 3.0 * (u + g * e) ** 2 * g * e + 1e-12 * u ** 3


def _drop(mat, self_offset):
    """column self_offset + i of row i -> 0 (a copy)"""
    mat = mat.clone()
    if self_offset >= 0:
        i = torch.arange(mat.shape[0], device=mat.device)
        mat[i, i + self_offset] = 0.0
    return mat


def _row_total(fn, a, b, gamma, coef0, self_offset, chunk=16384):
    """sum_j fn(a, b)_ij without column self_offset + i, the columns in chunks so that a large b never exists in fp64 as a whole"""
    gamma = _gamma(a, gamma)
    out = torch.zeros(a.shape[0], dtype=torch.float64, device=a.device)
    i = torch.arange(a.shape[0], device=a.device)
    for s in range(0, b.shape[0], chunk):
        mat = fn(a, b[s:s + chunk], gamma, coef0)
        if self_offset >= 0:
            j = i + self_offset - s
            ok = (j >= 0) & (j < mat.shape[1])
            mat[i[ok], j[ok]] = 0.0
        out += mat.sum(1)
    return out


def row_sums(a, b, gamma=None, coef0=1.0, self_offset=-1):
    """fp64 [na]: sum_j k_ij, column self_offset + i left out of row i"""
    return _row_total(kernel_matrix, a, b, gamma, coef0, self_offset)


def row_sum_bounds(a, b, gamma=None, coef0=1.0, self_offset=-1):
    return _row_total(delta_k, a, b, gamma, coef0, self_offset)


def _mmd2_of(fn, x, y, gamma, coef0, sign):
    m, n = x.shape[0], y.shape[0]
    sxx, syy = float(_drop(fn(x, x, gamma, coef0), 0).sum()), float(_drop(fn(y, y, gamma, coef0), 0).sum())
    sxy = float(fn(x, y, gamma, coef0).sum())
    return sxx / (m * (m - 1)) + syy / (n * (n - 1)) + sign * 2.0 * sxy / (m * n)


def mmd2(x, y, gamma=None, coef0=1.0):
    """the unbiased MMD^2 of x (m >= 2 rows) and y (n >= 2 rows) in fp64"""
    return _mmd2_of(kernel_matrix, x, y, gamma, coef0, -1.0)


def mmd2_bound(x, y, gamma=None, coef0=1.0):
    return _mmd2_of(delta_k, x, y, gamma, coef0, +1.0)


def block_bounds(m, n, max_block_size):
    """([(start, stop)] of the real set, the same of the generated one): n_blocks = ceil(max(m, n) / max_block_size) contiguous blocks each, the first
    n_blocks - p of v = size // n_blocks rows and the last p = size - v n_blocks of v + 1"""
    n_blocks = (max(m, n) + max_block_size - 1) // max_block_size
    out = []
    for size in (m, n):
        v = size // n_blocks
        p = size - v * n_blocks
        sizes = [v] * (n_blocks - p) + [v + 1] * p
        if min(sizes) < 2:
            raise ValueError("a block of fewer than 2 rows")
        starts = [sum(sizes[:b]) for b in range(n_blocks)]
        out.append([(s, s + z) for s, z in zip(starts, sizes)])
    return out[0], out[1]


def kid_blocks(x, y, max_block_size=1024, gamma=None, coef0=1.0):
    """dict(kid, std, n_blocks, est, kid_bound, std_bound, est_bounds): TF-GAN's block estimator in fp64 and the bounds above"""
    bx, by = block_bounds(x.shape[0], y.shape[0], max_block_size)
    B = len(bx)
    est = [mmd2(x[a0:a1], y[b0:b1], gamma, coef0) for (a0, a1), (b0, b1) in zip(bx, by)]
    bnd = [mmd2_bound(x[a0:a1], y[b0:b1], gamma, coef0) for (a0, a1), (b0, b1) in zip(bx, by)]
    mean = math.fsum(est) / B
    var = math.fsum((e - mean) ** 2 for e in est) / (B - 1) if B > 1 else 0.0
    std_bound = math.sqrt(math.fsum(v * v for v in bnd)) / math.sqrt(B * (B - 1)) if B > 1 else 0.0
    return dict(kid=mean, std=math.sqrt(var / B), n_blocks=B, est=est, kid_bound=math.fsum(bnd) / B, std_bound=std_bound, est_bounds=bnd)
