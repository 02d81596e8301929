"""numpy oracle of the coefficient fitter (naturaldiffusion_amd/fit.py; include/natinf_fit.h).  Not collected by pytest.

* ``gram``       -- the Gram matrix in np.longdouble, with the sum of |products| the error bound of any summation order is stated in;
* ``solve_row``  -- the constrained row problem through its bordered (Lagrange) system: another route than fit.py's elimination;
* ``TwoPoint``   -- the exact denoiser of per-element two-point data +-m on the VP schedule, x0 = m tanh(alpha m x / sigma^2);
* ``run`` / ``fit_sequential`` -- a deterministic Natural Inference trajectory and the row-by-row fit against a teacher, all in fp64."""
import numpy as np

from naturaldiffusion_amd import coeffgen


def gram(vectors, rounded=True):
    """vectors [M, E] (any float dtype, widened exactly) -> (G [M, M], S [M, M] = sum_e |v_a v_b|), accumulated in longdouble; ``rounded``: as fp64
    (one more rounding), else left in longdouble"""
    v = np.asarray(vectors).astype(np.longdouble)
    G, S = v @ v.T, np.abs(v) @ np.abs(v).T
    return (G.astype(np.float64), S.astype(np.float64)) if rounded else (G, S)


def gamma(n: int) -> float:
    u = n * 2.0 ** -53
    return u / (1.0 - u)


def solve_row(G, row_sum, b0=0.0, support=None, ridge=0.0):
    """minimise c' A c - 2 c' g over the supported columns, sum c = row_sum (None: free), via [[A, 1], [1', 0]] [c; lambda] = [g; row_sum] on the
    system scaled by A's diagonal"""
    G = np.asarray(G, np.float64)
    n = G.shape[0] - 2
    sup = list(range(n)) if support is None else sorted(int(j) for j in support)
    A = G[np.ix_(sup, sup)] + ridge * np.diag(np.diag(G)[sup])
    g = (G[:n, n + 1] - b0 * G[:n, n])[sup]
    d = np.sqrt(np.diag(A))
    As, gs = A / np.outer(d, d), g / d
    c = np.zeros(n)
    if row_sum is None:
        c[sup] = np.linalg.solve(As, gs) / d
        return c
    m = len(sup)
    K = np.zeros((m + 1, m + 1))
    K[:m, :m], K[:m, m], K[m, :m] = As, 1.0 / d, 1.0 / d
    c[sup] = np.linalg.solve(K, np.append(gs, row_sum))[:m] / d
    return c


class TwoPoint:
    """out = (x - alpha m tanh(alpha m x / sigma^2)) / sigma: the eps form of the exact denoiser of data +-m per element.  Called with numpy fp64 it is
    the oracle's model; called with torch tensors (x fp32 [B, ...], labels = t * 999) it is a ``model_fn``, evaluated in fp64 and rounded to fp32 once."""

    def __init__(self, m: float = 0.5):
        self.m = float(m)

    def x0(self, x, t):
        a, s = (float(v) for v in coeffgen.vp_alpha_sigma(t))
        return self.m * np.tanh(a * self.m * x / s ** 2)

    def __call__(self, x, labels):
        import torch
        t = float(labels[0]) / 999.0
        a, s = (float(v) for v in coeffgen.vp_alpha_sigma(t))
        xd = x.double()
        return ((xd - a * self.m * torch.tanh(a * self.m * xd / s ** 2)) / s).float()


def run(model: TwoPoint, C, B, node, noise, keep=None):
    """x_{k+1} = sum_j C[k, j] x0_j + B[k, 0] noise in fp64 -> (final state, {node index: state} for the indices in ``keep``, the x0 history)"""
    noise = np.asarray(noise, np.float64)
    x, hist, kept = noise, [], {}
    for k in range(C.shape[0]):
        hist.append(model.x0(x, node[k, 0]))
        x = sum(C[k, j] * hist[j] for j in range(k + 1)) + B[k, 0] * noise
        if keep is not None and k + 1 in keep:
            kept[k + 1] = x
    return x, kept, hist


def fit_sequential(model: TwoPoint, init, teacher, noise, order=None, t_tol=1e-6):
    """The sequential row fit in fp64 with the marginal constraint (row sum node[k+1, 1], B[k, 0] = node[k+1, 2]) -> (C, B, node)"""
    C0, B0, node = (np.asarray(a, np.float64) for a in init)
    tC, tB, tnode = (np.asarray(a, np.float64) for a in teacher)
    noise = np.asarray(noise, np.float64)
    n = C0.shape[0]
    match = {}
    for k in range(n):
        d = np.abs(tnode[:, 0] - node[k + 1, 0])
        assert d.min() <= t_tol
        match[k] = int(np.argmin(d))
    _, targets, _ = run(model, tC, tB, tnode, noise, keep=set(match.values()))
    C, B = C0.copy(), B0.copy()
    x, hist = noise, []
    for k in range(n):
        hist.append(model.x0(x, node[k, 0]))
        sup = list(range(k + 1)) if order is None else list(range(max(0, k + 1 - order), k + 1))
        V = np.stack([hist[j].reshape(-1) for j in sup] + [noise.reshape(-1), targets[match[k]].reshape(-1)])
        G = V @ V.T
        B[k, 0] = node[k + 1, 2]
        C[k] = 0.0
        C[k, sup] = solve_row(G, node[k + 1, 1], b0=B[k, 0])
        x = sum(C[k, j] * hist[j] for j in range(k + 1)) + B[k, 0] * noise
    return C, B, node


def final_mse(model: TwoPoint, students, teacher, noise):
    """mean squared difference of each student's final state to the teacher's final state (both end at the same time)"""
    tC, tB, tnode = teacher
    ref = run(model, tC, tB, tnode, noise)[0]
    return [float(np.mean((run(model, C, B, node, noise)[0] - ref) ** 2)) for C, B, node in students]
