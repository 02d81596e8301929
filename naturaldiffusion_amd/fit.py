"""Fit a Natural Inference coefficient matrix to a teacher run, one row at a time, by linear least squares on the HIP library's fp64 Gram kernel
(include/natinf_fit.h).

Row k of ``C`` is the combination of the student's own x0 predictions that lands closest to where a finer teacher run is at the same time node:

    minimise  sum_images | sum_j c_j x0_j + b0 noise - target |^2     subject to  sum_j c_j = row_sum ,

with x0_j the rows of the student's fp64 history, ``target`` the teacher's state and b0 = fp32(B[k, 0]), the value the fused step applies.  Every
quantity of that problem is an inner product between history rows, the noise and the target: one Gram matrix per image (``gram``), summed in ascending
image order (``sum_grams``), solved on the host (``solve_row``).  The Gram matrices of such histories reach condition numbers of 1e12, so everything here
is fp64 off the fp64 history.  The rows are fitted in sequence: row k sees the history the rows before it produced.

What a fit promises: each fitted row is optimal for its own Gram matrix -- on the fitting images, given the rows before it.  It does not promise a
smaller error on other images or at the final node than the matrix it started from; ``CIFAR10NaturalInference.fit_coeff_matrix`` measures that on
held-out images.

This module imports without the library; everything except ``gram`` (and what calls it) is host code."""
from __future__ import annotations

import ctypes
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from .coeff import is_stochastic

MAX_ROWS = 30                         # include/natinf_fit.h: NATINF_FIT_MAX_ROWS
MAX_EPI, MAX_IMAGES = 1 << 24, 1 << 20
CONSTRAINTS = ("marginal", "init", None)


def _lib():
    from . import _lib as L
    return L


# ---- the kernel ----

def gram(hist: torch.Tensor, rows: Sequence[int], noise: torch.Tensor, target: torch.Tensor, n_images: int, elems_per_image: int,
         first_image: int = 0) -> torch.Tensor:
    """fp64 [n_images, M, M] on the device, M = len(rows) + 2: per image the Gram matrix of the history rows ``rows`` (strictly ascending slots of
    ``hist``, an fp64 [n_slot, E] slab read in place), the image's ``noise`` and its ``target`` (fp32, ``E`` or more elements each, image i at
    ``i * elems_per_image``), for the images ``first_image .. first_image + n_images - 1`` of the slab.  An image's matrix is the same bytes however the
    images are split over calls."""
    rows = [int(r) for r in rows]
    n, epi, first = int(n_images), int(elems_per_image), int(first_image)
    if not 1 <= len(rows) <= MAX_ROWS or rows[0] < 0 or any(b <= a for a, b in zip(rows, rows[1:])):
        raise ValueError(f"fit: rows must be 1..{MAX_ROWS} strictly ascending non-negative history slots")
    if epi < 4 or epi % 4 or epi > MAX_EPI or not 1 <= n <= MAX_IMAGES or first < 0:
        raise ValueError("fit: elems_per_image must be a multiple of 4 in 4..2^24, n_images in 1..2^20, first_image >= 0")
    if not (isinstance(hist, torch.Tensor) and hist.dtype == torch.float64 and hist.dim() == 2 and hist.is_contiguous() and hist.is_cuda):
        raise ValueError("fit: hist must be a contiguous fp64 [n_slot, E] tensor on the device")
    if rows[-1] >= hist.shape[0] or hist.shape[1] < (first + n) * epi or hist.shape[1] % 2:
        raise ValueError("fit: rows / images outside the history slab (or a slab of odd row length)")
    for name, t in (("noise", noise), ("target", target)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous() and t.device == hist.device and t.numel() >= (first + n) * epi):
            raise ValueError(f"fit: {name} must be a contiguous fp32 tensor on the history's device holding every image of the call")
    L = _lib()
    M = len(rows) + 2
    out = torch.empty((n, M, M), dtype=torch.float64, device=hist.device)
    rows_c = (ctypes.c_int32 * len(rows))(*rows)
    with torch.cuda.device(hist.device):
        L.check(L.lib.natinf_fit_gram_f64(L.ptr(hist) + 8 * first * epi, int(hist.shape[1]), rows_c, len(rows), L.ptr(noise) + 4 * first * epi,
                                          L.ptr(target) + 4 * first * epi, n, epi, L.ptr(out), L.stream_ptr()), "natinf_fit_gram_f64")
    return out


# ---- host code ----

def sum_grams(per_image) -> np.ndarray:
    """fp64 [M, M]: the per-image matrices ([n, M, M]: a tensor, an array, or a sequence of such batches) added one image after the other in ascending
    order, so the sum is the same for any batching."""
    parts = per_image if isinstance(per_image, (list, tuple)) else [per_image]
    acc = None
    for p in parts:
        p = np.asarray(p.detach().cpu() if isinstance(p, torch.Tensor) else p, dtype=np.float64)
        if p.ndim != 3 or p.shape[1] != p.shape[2]:
            raise ValueError("fit: per-image Gram matrices are [n, M, M]")
        for g in p:
            acc = g.copy() if acc is None else acc + g
    if acc is None:
        raise ValueError("fit: no Gram matrix to sum")
    return acc


def _blocks(G, b0: float):
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 3:
        raise ValueError("fit: a Gram matrix is [M, M] with M = history rows + 2 (noise, target)")
    n = G.shape[0] - 2
    return G, n, G[:n, :n], G[:n, n + 1] - float(b0) * G[:n, n]


def _scaled_solve(H: np.ndarray, rhs: np.ndarray):
    """H y = rhs through the system scaled to a unit diagonal -> (y, condition number of the scaled system)"""
    d = np.sqrt(np.abs(np.diag(H)))
    d = np.where(d > 0, d, 1.0)
    Hs = H / np.outer(d, d)
    try:
        y = np.linalg.solve(Hs, rhs / d)
    except np.linalg.LinAlgError:
        y = np.linalg.lstsq(Hs, rhs / d, rcond=None)[0]
    return y / d, float(np.linalg.cond(Hs))


def solve_row(G, row_sum: Optional[float], *, b0: float = 0.0, support: Optional[Sequence[int]] = None, ridge: float = 0.0, return_cond: bool = False):
    """The coefficients c (fp64 [n]) that minimise c' G_hh c - 2 c' g over the columns in ``support`` (default: all), with G_hh the history block of the
    Gram matrix ``G`` ([n + 2, n + 2]; row n the noise, row n + 1 the target) and g = G[:n, target] - ``b0`` * G[:n, noise]: the least-squares fit of
    sum_j c_j v_j + b0 noise to the target.  ``row_sum``: the value sum_j c_j must have (the last supported coefficient is eliminated, so it holds to
    rounding), or None for no constraint.  ``ridge`` adds ridge * diag(G_hh).  The system is scaled to a unit diagonal before it is solved.
    Unsupported columns are exact zeros."""
    G, n, A, g = _blocks(G, b0)
    if ridge < 0 or not np.isfinite(ridge):
        raise ValueError("fit: ridge must be finite and >= 0")
    sup = list(range(n)) if support is None else sorted({int(j) for j in support})
    if not sup or sup[0] < 0 or sup[-1] >= n:
        raise ValueError("fit: support must name at least one history column")
    A = A[np.ix_(sup, sup)] + float(ridge) * np.diag(np.diag(A)[sup])
    g = g[sup]
    c = np.zeros(n)
    if row_sum is None:
        y, cond = _scaled_solve(A, g)
        c[sup] = y
    elif len(sup) == 1:
        c[sup[0]], cond = float(row_sum), 1.0
    else:
        # c = row_sum e_p + Z y with p the last supported column and the columns of Z the differences e_j - e_p: Z' A Z y = Z' (g - row_sum A e_p)
        m = len(sup) - 1
        Z = np.vstack([np.eye(m), -np.ones((1, m))])
        y, cond = _scaled_solve(Z.T @ A @ Z, Z.T @ (g - float(row_sum) * A[:, m]))
        c[sup[:-1]] = y
        c[sup[-1]] = float(row_sum) - float(np.sum(y))
    return (c, cond) if return_cond else c


def row_residual(G, c, b0: float) -> float:
    """| sum_j c_j v_j + b0 noise - target |^2 from the Gram matrix alone: w' G w with w = (c, b0, -1), evaluated in extended precision (the value is a
    difference of far larger terms; what remains is the rounding of G's own entries)"""
    G = np.asarray(G, dtype=np.float64)
    w = np.concatenate([np.asarray(c, np.float64).reshape(-1), [float(b0), -1.0]]).astype(np.longdouble)
    if G.ndim != 2 or G.shape != (w.size, w.size):
        raise ValueError("fit: c must have one coefficient per history row of G")
    return float(w @ (G.astype(np.longdouble) @ w))


def _triple(t, what: str):
    try:
        C, B, node = (np.asarray(a, dtype=np.float64) for a in t)
    except (TypeError, ValueError):
        raise ValueError(f"fit: {what} must be a (C, B, node) triple") from None
    n = C.shape[0] if C.ndim == 2 else -1
    if n < 1 or C.shape != (n, n) or B.ndim != 2 or B.shape[0] != n or B.shape[1] < 1 or node.shape != (n + 1, 3):
        raise ValueError(f"fit: {what} has inconsistent shapes C{C.shape} B{B.shape} node{node.shape}")
    if is_stochastic(B):
        raise ValueError(f"fit: {what} is a stochastic matrix (B[k, j >= 1] != 0); only deterministic students and teachers are fitted")
    if np.any(np.triu(C, 1) != 0):
        raise ValueError(f"fit: {what}'s C must be lower triangular")
    return C, B, node


def match_nodes(node: np.ndarray, teacher_node: np.ndarray, ks: Sequence[int], t_tol: float = 1e-6) -> dict:
    """{k: m}: for every row k the teacher node m whose time is within ``t_tol`` of node[k + 1, 0] (the state x_{k+1} is compared with the teacher's
    state at node m, the output of its step m - 1); a row without one is a ValueError"""
    out = {}
    tt = np.asarray(teacher_node, np.float64)[:, 0]
    for k in ks:
        d = np.abs(tt - float(node[k + 1, 0]))
        m = int(np.argmin(d))
        if not d[m] <= t_tol or m < 1:
            raise ValueError(f"fit: row {k} ends at t = {node[k + 1, 0]!r}, and the teacher has no node within {t_tol} of it (nearest: {tt[m]!r})")
        out[int(k)] = m
    return out


def _support(k: int, order: Optional[int]) -> list:
    return list(range(k + 1)) if order is None else list(range(max(0, k + 1 - order), k + 1))


def _check_fit_args(init, teacher, rows, order, ridge, constraint, batch_size, t_tol):
    C0, B0, node = _triple(init, "init")
    teacher = _triple(teacher, "teacher")
    n = C0.shape[0]
    if order is not None and (isinstance(order, bool) or int(order) != order or order < 1):
        raise ValueError("fit: order must be None or an integer >= 1")
    order = None if order is None else int(order)
    ks = list(range(n)) if rows is None else sorted({int(k) for k in rows})
    if not ks or ks[0] < 0 or ks[-1] >= n:
        raise ValueError(f"fit: rows must name rows 0..{n - 1} of the student")
    if constraint not in CONSTRAINTS:
        raise ValueError('fit: constraint must be "marginal", "init" or None')
    if not (np.isfinite(ridge) and ridge >= 0):
        raise ValueError("fit: ridge must be finite and >= 0")
    if int(batch_size) < 1:
        raise ValueError("fit: batch_size must be >= 1")
    if not t_tol >= 0:
        raise ValueError("fit: t_tol must be >= 0")
    wide = [k for k in ks if len(_support(k, order)) > MAX_ROWS]
    if wide:
        raise ValueError(f"fit: row {wide[0]} has more than {MAX_ROWS} supported columns; give order <= {MAX_ROWS}")
    return (C0, B0, node), teacher, ks, order, match_nodes(node, teacher[2], ks, t_tol)


def _check_noise(noise) -> int:
    if not isinstance(noise, torch.Tensor) or noise.dtype != torch.float32 or noise.dim() < 2 or noise.shape[0] < 1:
        raise ValueError("fit: noise must be an fp32 tensor [n_images, ...]")
    epi = noise.numel() // noise.shape[0]
    if epi < 4 or epi % 4 or epi > MAX_EPI:
        raise ValueError("fit: an image must hold a multiple of 4 values, 4..2^24")
    return epi


def _labels(ni, k: int, n: int) -> torch.Tensor:
    return torch.full((n,), ni.labels[k], dtype=torch.float32, device=ni.device)


def teacher_states(model_fn: Callable, teacher, noise: torch.Tensor, wanted: Sequence[int], seed=None) -> dict:
    """{m: the teacher's state at node m, fp32 like ``noise``} for the nodes in ``wanted`` (1..N): one ``CifarNI`` trajectory on ``noise``, stepped as
    ``CifarNI.run`` steps it and stopped at the last wanted node; only the wanted states are kept"""
    from .sampler import CifarNI
    C, B, node = teacher
    ni = CifarNI(C, B, node, noise.numel(), device=noise.device, seed=seed)
    shape, flat = noise.shape, noise.reshape(-1)
    x, keep = flat, {}
    for m in range(max(wanted)):
        out = model_fn(x.view(shape), _labels(ni, m, shape[0]))
        x = ni.step(m, x.reshape(-1), out.contiguous().reshape(-1), flat)
        if m + 1 in wanted:
            keep[m + 1] = x.clone().view(shape)
    return keep


@torch.no_grad()
def fit_matrix(model_fn: Callable, init, teacher, noise: torch.Tensor, *, rows: Optional[Sequence[int]] = None, order: Optional[int] = None,
               ridge: float = 0.0, constraint: Optional[str] = "marginal", batch_size: int = 256, t_tol: float = 1e-6, seed: Optional[int] = None):
    """(C, B, node, report): ``init`` with the rows in ``rows`` (default: all) fitted, in ascending order, to ``teacher``'s trajectory on ``noise``
    (fp32 [n_images, ...] on the device: x_0 of both).  ``init`` and ``teacher`` are deterministic (C, B, node) triples; the student's nodes are
    ``init``'s, and every fitted row k needs a teacher node within ``t_tol`` of node[k + 1, 0].  ``order=p`` supports the last p columns of a row only
    (those are the only history rows the kernel reads, so a long student fits within 30 columns); other columns of a fitted row are exact zeros.

    ``constraint``: ``"marginal"`` -- row sum node[k + 1, 1] and B[k, 0] = node[k + 1, 2], as the shipped ``weights/step_*`` have; ``"init"`` -- the
    init row's own sum and B[k, 0]; ``None`` -- no constraint on the sum, B[k, 0] from ``init``.

    Per row every batch (its own ``CifarNI``, whose history is n_step * E * 8 bytes) pushes x0_k into its history through the ordinary ``CifarNI.step``;
    the Gram matrices of all batches are summed, the row is solved once and applied through the same ``CifarNI.step``, so ``CifarNI.run`` with the
    returned matrix on the same noise reproduces ``report["x_final"]`` byte for byte.

    ``report``: ``rows`` -- per fitted row a dict(row, support, row_sum, b0, residual, init_residual (Gram residuals of the fitted and of the init row
    over all images; the latter NaN when the init row has coefficients outside the support), mse, init_mse (measured: mean squared difference of
    x_{k+1} to the target under the fitted and under the init row), target_ms (the target's mean square), cond (condition number of the scaled system), teacher_node); ``x_final`` -- the
    student's final states, fp32 like ``noise``."""
    (C0, B0, node), teacher, ks, order, match = _check_fit_args(init, teacher, rows, order, ridge, constraint, batch_size, t_tol)
    epi = _check_noise(noise)
    from .coeff import SparseRows
    from .sampler import CifarNI
    _lib().require_gpu()
    noise = noise.contiguous()
    n_img, n_step, shape1 = int(noise.shape[0]), C0.shape[0], tuple(noise.shape[1:])
    C, B = C0.copy(), B0.copy()
    batches = []
    for s in range(0, n_img, int(batch_size)):
        nz = noise[s:s + int(batch_size)]
        ni = CifarNI(C, B, node, nz.numel(), device=noise.device, seed=seed)
        batches.append(dict(ni=ni, noise=nz.reshape(-1), shape=nz.shape, n=int(nz.shape[0]), x=nz.reshape(-1),
                            targets=teacher_states(model_fn, teacher, nz, sorted(set(match.values())), seed=seed)))
    report = []
    for k in range(n_step):
        fitted = k in match
        for b in batches:
            ni = b["ni"]
            out = model_fn(b["x"].view(b["shape"]), _labels(ni, k, b["n"])).contiguous().reshape(-1)
            b["next"] = ni.step(k, b["x"], out, b["noise"])             # x0_k enters the history; x_{k+1} under the init row
            b["out"] = out if fitted else None
        if fitted:
            sup = _support(k, order)
            tgt = [b["targets"][match[k]].reshape(-1) for b in batches]
            G = sum_grams([gram(b["ni"].hist, sup, b["noise"], t, b["n"], epi) for b, t in zip(batches, tgt)])
            if constraint == "marginal":
                row_sum, B[k, 0] = float(node[k + 1, 1]), node[k + 1, 2]
            else:
                row_sum = float(np.sum(C0[k])) if constraint == "init" else None
            b0 = float(np.float32(B[k, 0]))                             # what the fused step multiplies the noise with
            c, cond = solve_row(G, row_sum, b0=b0, ridge=ridge, return_cond=True)
            outside = np.delete(C0[k], sup)
            init_res = row_residual(G, C0[k, sup], float(np.float32(B0[k, 0]))) if not np.any(outside != 0) else float("nan")
            sq = lambda key: sum(float((b[key].double() - t.double()).pow(2).sum()) for b, t in zip(batches, tgt)) / (n_img * epi)
            init_mse = sq("next")
            C[k] = 0.0
            C[k, sup] = c
            for b in batches:                                           # the fitted row through the same step: x0_k is recomputed to the same bytes
                ni = b["ni"]
                ni.C, ni.B = C, B
                ni.rows = SparseRows(C, lambda r: r + 1, torch.float64, ni.device)
                b["next"] = ni.step(k, b["x"], b["out"], b["noise"])
                b["out"] = None
            report.append(dict(row=k, support=sup, row_sum=row_sum, b0=b0, residual=row_residual(G, c, b0), init_residual=init_res, mse=sq("next"),
                               init_mse=init_mse, target_ms=float(G[-1, -1]) / (n_img * epi), cond=cond, teacher_node=match[k]))
        for b in batches:
            b["x"] = b["next"]
    x_final = torch.cat([b["x"].view(b["shape"]) for b in batches]).clone()
    return C, B, node, dict(rows=report, x_final=x_final)


@torch.no_grad()
def final_mse(model_fn: Callable, students, teacher, noise: torch.Tensor, *, batch_size: int = 256, t_tol: float = 1e-6, seed: Optional[int] = None) -> list:
    """The mean squared difference of every student's final state (``students``: (C, B, node) triples with the same last node) to the teacher's state at
    the matching node, on ``noise`` -- one float per student"""
    students = [_triple(s, "a student") for s in students]
    teacher = _triple(teacher, "teacher")
    ms = {match_nodes(s[2], teacher[2], [s[0].shape[0] - 1], t_tol)[s[0].shape[0] - 1] for s in students}
    if len(ms) != 1:
        raise ValueError("fit: the students end at different teacher nodes")
    m = ms.pop()
    _check_noise(noise)
    from .sampler import CifarNI
    _lib().require_gpu()
    noise = noise.contiguous()
    sums = [0.0] * len(students)
    for s in range(0, noise.shape[0], int(batch_size)):
        nz = noise[s:s + int(batch_size)]
        tgt = teacher_states(model_fn, teacher, nz, [m], seed=seed)[m].double()
        for i, (C, B, node) in enumerate(students):
            x = CifarNI(C, B, node, nz.numel(), device=nz.device, seed=seed).run(model_fn, nz)
            sums[i] += float((x.double() - tgt).pow(2).sum())
    return [v / noise.numel() for v in sums]
