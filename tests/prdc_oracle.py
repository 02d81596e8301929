"""fp64 definition of the k-nearest-neighbour manifold metrics (include/natinf_prdc.h; naturaldiffusion_amd/prdc.py) in plain torch, and the test inputs.

Inputs are low-dimensional clusters pushed through a fixed random map, so that neighbour gaps are wide: X = 0.5 relu(Z W + 0.3 E), Z ~ N(shift, 1) of shape
[n, 6], W fixed [6, d].  (Isotropic Gaussians in d dimensions are not usable: their distances concentrate and many rows sit within rounding of a radius.)"""
import torch

INF = float("inf")


def cluster_feats(n, d, shift, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(6, d, generator=torch.Generator().manual_seed(1234), dtype=torch.float64)
    Z = torch.randn(n, 6, generator=g, dtype=torch.float64) + shift
    E = torch.randn(n, d, generator=g, dtype=torch.float64)
    return (0.5 * torch.relu(Z @ W + 0.3 * E)).float()


def dist2(a, b):
    """fp64 [na, nb] squared distances of fp32 rows: |a|^2 + |b|^2 - 2 a.b with every step in fp64 (error about 1e-15 of the norms), the columns in
    chunks so that a large b never exists in fp64 as a whole"""
    a = a.double()
    na = (a ** 2).sum(1)
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float64, device=a.device)
    for s in range(0, b.shape[0], 16384):
        bc = b[s:s + 16384].double()
        out[:, s:s + 16384] = (na[:, None] + (bc ** 2).sum(1)[None, :] - 2.0 * (a @ bc.t())).clamp_min(0.0)
    return out


def norm_sums(a, b):
    """|a_i|^2 + |b_j|^2: the scale of the distance kernels' error"""
    return (a.double() ** 2).sum(1)[:, None] + (b.double() ** 2).sum(1)[None, :]


def mask_self(d2, self_offset):
    """column self_offset + i of row i -> +inf (a copy)"""
    d2 = d2.clone()
    if self_offset >= 0:
        i = torch.arange(d2.shape[0], device=d2.device)
        d2[i, i + self_offset] = INF
    return d2


def kth(d2, k):
    return d2.kthvalue(k, dim=1).values


def radii(x, k):
    return kth(mask_self(dist2(x, x), 0), k)


def counts(d2, r2_rows, r2_cols):
    """(cnt_row_ball, cnt_col_ball) of a distance matrix"""
    return (d2 <= r2_rows[:, None]).sum(1), (d2 <= r2_cols[None, :]).sum(1)


def count_interval(d2, band, r2_rows, r2_cols, band_r2_rows, band_r2_cols):
    """(lo, hi) of both counts when every d2 may be off by `band` [rows, cols] and every radius by its own band"""
    lo = counts(d2 + band, r2_rows - band_r2_rows, r2_cols - band_r2_cols)
    hi = counts(d2 - band, r2_rows + band_r2_rows, r2_cols + band_r2_cols)
    return lo, hi


def prdc(real, gen, k):
    """the four numbers in fp64"""
    r2_real, r2_gen = radii(real, k), radii(gen, k)
    d_gr = dist2(gen, real)
    g = (d_gr <= r2_real[None, :]).sum(1)
    d_rg = d_gr.t()
    r = (d_rg <= r2_gen[None, :]).sum(1)
    o = (d_rg <= r2_real[:, None]).sum(1)
    return dict(precision=float((g > 0).double().mean()), recall=float((r > 0).double().mean()),
                density=float(g.double().mean()) / k, coverage=float((o > 0).double().mean()))
