"""fp64 numpy restatement of the ideal denoiser's definition (include/natinf_ideal.h), for tests/test_ideal_host.py and tests/test_gpu_ideal.py.

    z_ij  = d2_ij == +inf ? -inf : -(c_i d2_ij)          m_i = max_j z_ij        lse_i = m_i + log(sum_j exp(z_ij - m_i))
    p_ij  = exp(z_ij - lse_i)                            mean_i = sum_j p_ij f_j
    pmax_i = exp(m_i - lse_i)                            nearest_i = the lowest j with the smallest d2_ij (chosen on d2, not on z)
    out_i = (x_i - alpha_i mean_i) / sigma_i

``d2`` is either formed here, exactly as |u - f|^2 in fp64, or handed in (the device's own table).  Summation orders are numpy's: the tests' bounds
are far above an fp64 sum's order dependence."""
import numpy as np


def dist2(u, f, self_offset=-1):
    """fp64 [B, N]: the sum of squared differences, row by row; column self_offset + i of row i is +inf"""
    u, f = np.asarray(u, np.float64), np.asarray(f, np.float64)
    d2 = np.stack([((r[None, :] - f) ** 2).sum(1) for r in u])
    return leave_out(d2, self_offset)


def leave_out(d2, self_offset=-1):
    d2 = np.array(d2, dtype=np.float64)
    if self_offset >= 0:
        d2[np.arange(len(d2)), self_offset + np.arange(len(d2))] = np.inf
    return d2


def logits(d2, c):
    d2 = np.asarray(d2, np.float64)
    c = np.broadcast_to(np.asarray(c, np.float64), (d2.shape[0],))[:, None]
    with np.errstate(invalid="ignore"):
        z = -(c * d2)
    return np.where(np.isinf(d2), -np.inf, z)             # a select: 0 * inf never reaches the softmax


def softmax_stats(d2, c):
    """dict(p [B, N], lse, pmax, m [B] fp64, nearest [B] int64) of a distance table"""
    z = logits(d2, c)
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    return dict(p=np.exp(z - lse[:, None]), lse=lse, pmax=np.exp(m - lse), m=m, nearest=np.argmin(np.asarray(d2, np.float64), axis=1))


def posterior_mean(u, c, f, self_offset=-1, d2=None, x=None, alpha=None, sigma=None):
    """dict(x0 fp64 [B, d] (unrounded), p, lse, pmax, nearest, and out with x / alpha / sigma)"""
    f = np.asarray(f, np.float64)
    st = softmax_stats(dist2(u, f, self_offset) if d2 is None else d2, c)
    st["x0"] = st["p"] @ f
    if x is not None:
        B = len(st["x0"])
        a = np.broadcast_to(np.asarray(alpha, np.float64), (B,))[:, None]
        s = np.broadcast_to(np.asarray(sigma, np.float64), (B,))[:, None]
        st["out"] = (np.asarray(x, np.float64) - a * st["x0"]) / s
    return st


def step_x0(out, x, alpha, sigma, std):
    """natinf_step_f64hist's x0 from a network output: ((-out / std) sigma^2 + x) / alpha in fp64"""
    return ((-np.asarray(out, np.float64) / std) * sigma ** 2 + np.asarray(x, np.float64)) / alpha
