"""fp64 definition of the Inception Score's row statistics (include/natinf_is.h; naturaldiffusion_amd/iscore.py) in plain torch, the test inputs, and the
bounds on what the device may differ from fp64 by.

Inputs (``case``).  Features are prdc_oracle.cluster_feats(n, d, shift, 2).  The head's weights are N(0, 1), scaled so that the logits of the case's
features have standard deviation 2.5 (root mean square where there is a single logit); the bias is 0.5 N(0, 1) - 20.  For the planted classes
{0, 31, 32, 63, 64, 127, 128, C - 113, C - 112, C - 2, C - 1} within [0, C), in ascending order, the k-th is planted on row 5 k + 3 (where the case has
that row): coordinate 5 k + 1 is made private -- zero in every other row and every other class -- and a[5 k + 3, 5 k + 1] = 8, W[c_k, 5 k + 1] = 3, which
adds 24 to one logit of one row.  A planted class is its row's largest by far, so a kernel that drops, doubles or misplaces a class at a tile edge (0,
31 | 32, 63 | 64, 127 | 128, the last tile's ends) moves that row's log-sum-exp by thousands of bounds.  The bias offset -20 shifts every logit alike and
changes no probability; it puts the log-sum-exp of every row without a planted class below -2.5 (-6 at d = 2048), so that a padding column of the
staged logits read as z = 0 would move it by more than 2.5: tens of thousands of bounds.

Bounds: derived, not measured on the code under test.  The dot product is the distance kernels' own, whose band on s_ij (kid_oracle.E_REL, half of
tests/test_gpu_prdc.py's BAND on d2) is

    e_ij = 2^-22 (|a_i|^2 + |w_j|^2),        E_i = max_j e_ij.

The bias is added in fp64 and everything after it is fp64 with a few thousand roundings of 2^-53 at the most; the terms 1e-12 (...) stand for those.

    bound(lse_i)   = E_i + 1e-12 (1 + |lse_i|)
        log-sum-exp is 1-Lipschitz in the largest logit error (its gradient is p, |p|_1 = 1).
    bound(h_i)     = E_i e^{2 E_i} (S_i + 4 E_i) + 1e-12 (1 + |h_i|),        S_i = sum_j p_ij |log p_ij - h_i|
        h = sum_j p_j log p_j has dh/dz_j = p_j (log p_j - h).  By the mean value theorem |dh| <= E max over the segment of sum_j p_j |log p_j - h|.
        Along the segment every z_j moves by at most E and lse by at most E: log p_j by at most 2 E and p_j by a factor of at most e^{2 E}; the term
        4 E allows |log p_j - h| to move by 2 E for log p_j and 2 E for h.  (h itself moves by E S_i to first order, so the allowance for h is exact only
        where S_i <= 2; the term is of second order in E <= 1e-3 either way, 1e-3 of the bound at the most.)
    dpbar_j        = mean_i((e^{2 E_i} - 1) p_ij) + 2^-43 + 1e-12 pbar_j
        p_ij moves by the factor above; every q_ij = llrint(2^42 p_ij) is within 1/2 of 2^42 p_ij, that is 2^-43 of p_ij, and so is their mean.
    bound(log IS)  = mean_i bound(h_i) + sum_j (what x log x moves by over [max(pbar_j - dpbar_j, 0), pbar_j + dpbar_j])
        where the interval stays above 0: dpbar_j max |1 + log x| over it (the derivative is monotone: an end of the interval); where it reaches 0: the
        range of x log x on it.
    a split's score s_k = exp(log IS_k) moves by ds_k <= s_k (e^{bound_k} - 1); their mean by mean_k ds_k; their population standard deviation
    |s - mean|_2 / sqrt(K) by |ds|_2 / sqrt(K): centring is a projection (it lengthens no vector), and the norm of a vector moves by no more than the norm
    of what is added to it (kid_oracle's argument)."""
import math

import torch

import kid_oracle as KO
import prdc_oracle as O

E_REL = KO.E_REL
FRAC_BITS = 42
ONE = float(1 << FRAC_BITS)


def planted_classes(C):
    return sorted({c for c in (0, 31, 32, 63, 64, 127, 128, C - 113, C - 112, C - 2, C - 1) if 0 <= c < C})


def case(n, C, d, seed=0, shift=0.6, offset=-20.0):
    """dict(a fp32 [n, d], W fp32 [C, d], b fp32 [C], planted [(class, row)])"""
    a = O.cluster_feats(n, d, shift, 2).clone()
    g = torch.Generator().manual_seed(7000 + seed)
    W = torch.randn(C, d, generator=g, dtype=torch.float64)
    b = (0.5 * torch.randn(C, generator=g, dtype=torch.float64) + offset).float()
    plants = [(c, 5 * k + 3, 5 * k + 1) for k, c in enumerate(planted_classes(C)) if 5 * k + 3 < n and 5 * k + 1 < d]
    for _, _, col in plants:
        a[:, col] = 0.0
        W[:, col] = 0.0
    z = a.double() @ W.t()
    spread = float(z.std(unbiased=False)) if z.numel() > 1 else 0.0
    spread = spread if spread > 0.0 else float(z.pow(2).mean().sqrt())
    W = (W * (2.5 / spread)).float()
    for c, row, col in plants:
        a[row, col] = 8.0
        W[c, col] = 3.0
    return dict(a=a, W=W, b=b, planted=[(c, row) for c, row, _ in plants])


def logits(a, W, b=None):
    z = a.double() @ W.double().t()
    return z if b is None else z + b.double()[None, :]


def row_stats(z):
    """dict(m, lse, logp, p, h, top, gap) of fp64 logits [n, C]; gap: the largest logit minus the second largest (inf for one class)"""
    m, top = z.max(1)
    lse = m + torch.log(torch.exp(z - m[:, None]).sum(1))
    logp = z - lse[:, None]
    p = torch.exp(logp)
    h = (p * logp).sum(1)
    if z.shape[1] > 1:
        two = z.topk(2, dim=1).values
        gap = two[:, 0] - two[:, 1]
    else:
        gap = torch.full_like(m, float("inf"))
    # torch.max returns some index of the maximum: the definition is the lowest
    top = (z == m[:, None]).int().argmax(1)
    return dict(m=m, lse=lse, logp=logp, p=p, h=h, top=top, gap=gap)


def row_error(a, W):
    """E_i fp64 [n]"""
    return E_REL * ((a.double() ** 2).sum(1) + (W.double() ** 2).sum(1).max())


def log_score(p):
    """log IS of the rows of p (fp64 [n, C]) in fp64"""
    pbar = p.mean(0)
    logp = torch.where(p > 0, torch.log(p.clamp_min(1e-300)), torch.zeros_like(p))
    h = (p * logp).sum(1)
    nz = pbar > 0
    return float(h.mean() - (pbar[nz] * torch.log(pbar[nz])).sum())


def _xlogx(x):
    return x * math.log(x) if x > 0.0 else 0.0


def _xlogx_moves(pbar, dp):
    lo, hi = max(pbar - dp, 0.0), pbar + dp
    if lo > 0.0:
        return dp * max(abs(1.0 + math.log(lo)), abs(1.0 + math.log(hi)))
    vals = [0.0, _xlogx(hi)] + ([-1.0 / math.e] if hi >= 1.0 / math.e else [])
    return max(vals) - min(vals)


def bounds(a, W, b=None):
    """dict of the fp64 values and the bounds of the set a under the head (W, b): E, lse, h, top, gap, p, lse_bound, h_bound, pbar, dpbar, log_is,
    log_is_bound, q (2^42 sum_i p_ij, fp64) and q_bound"""
    st = row_stats(logits(a, W, b))
    E = row_error(a, W)
    n = a.shape[0]
    S = (st["p"] * (st["logp"] - st["h"][:, None]).abs()).sum(1)
    h_bound = E * torch.exp(2 * E) * (S + 4 * E) + 1e-12 * (1 + st["h"].abs())
    lse_bound = E + 1e-12 * (1 + st["lse"].abs())
    pbar = st["p"].mean(0)
    dpbar = (torch.expm1(2 * E)[:, None] * st["p"]).mean(0) + 2.0 ** -(FRAC_BITS + 1) + 1e-12 * pbar
    moved = math.fsum(_xlogx_moves(float(x), float(dx)) for x, dx in zip(pbar.tolist(), dpbar.tolist()))
    return dict(E=E, lse=st["lse"], h=st["h"], top=st["top"], gap=st["gap"], p=st["p"], lse_bound=lse_bound, h_bound=h_bound, pbar=pbar, dpbar=dpbar,
                log_is=log_score(st["p"]), log_is_bound=float(h_bound.mean()) + moved, q=ONE * st["p"].sum(0), q_bound=n * ONE * dpbar)


def split_bounds(n, splits):
    return [(k * n // splits, (k + 1) * n // splits) for k in range(splits)]


def score_splits(a, W, b=None, splits=1):
    """dict(is, std, log_is, is_bound, std_bound, log_is_bounds): the splits protocol in fp64 and the bounds above"""
    parts = [bounds(a[s:e], W, b) for s, e in split_bounds(a.shape[0], splits)]
    log_is, bnd = [p["log_is"] for p in parts], [p["log_is_bound"] for p in parts]
    s = [math.exp(v) for v in log_is]
    ds = [v * math.expm1(e) for v, e in zip(s, bnd)]
    mean = math.fsum(s) / splits
    std = math.sqrt(math.fsum((v - mean) ** 2 for v in s) / splits) if splits > 1 else None
    return dict(**{"is": mean}, std=std, log_is=log_is, is_bound=math.fsum(ds) / splits,
                std_bound=math.sqrt(math.fsum(v * v for v in ds)) / math.sqrt(splits) if splits > 1 else None, log_is_bounds=bnd)


def lse_without(z, col):
    """fp64 [n]: the log-sum-exp of every row with column `col` left out (C >= 2)"""
    keep = torch.ones(z.shape[1], dtype=torch.bool)
    keep[col] = False
    return torch.logsumexp(z[:, keep], dim=1)


def lse_with_zero_column(z):
    """fp64 [n]: the log-sum-exp of every row with one column z = 0 appended"""
    return torch.logsumexp(torch.cat([z, torch.zeros(z.shape[0], 1, dtype=z.dtype)], dim=1), dim=1)
