"""The ideal (empirical-Bayes) denoiser on the HIP library's exact distance sweep (include/natinf_ideal.h): the posterior mean
over a training set,

    x0_i = sum_j p_ij f_j ,   p_ij = softmax_j(-c_i |u_i - f_j|^2) ,

which for u = x_t / alpha and c = alpha^2 / (2 sigma^2) is E[x0 | x_t] under x_t = alpha f + sigma eps and a uniform prior on the training rows -- the
exact minimum-MSE denoiser of the empirical training distribution.  It is the weighted sum whose concentration ``posterior_stats`` measures, the optimum a
trained network's x0 prediction is compared with, and -- as a ``model_fn`` -- a sampler that is known to copy its training set: the positive control of
``neighbours.nearest``'s memorisation audit.

Every output of a row depends on that row, its scalars and the training set only: the rows split freely over calls and ranks, the same bytes.

This module imports without the library (``level_scalars``, ``levels_of_labels`` and the argument checks are host code); everything else needs the GPU."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .prdc import FeatureSet, _lib

K_RANGE, CHUNK_ROWS = 2048, 256      # include/natinf_ideal.h: NATINF_IDEAL_K_RANGE, NATINF_IDEAL_CHUNK_ROWS
MAX_D, MAX_N = 4096, 1 << 20         # include/natinf_prdc.h


def padded_cols(n: int) -> int:
    """Np: the row length of the transposed planes and of the weight planes"""
    return (int(n) + 63) // 64 * 64


def check_width(d: int) -> None:
    if d % 64 or not (64 <= d <= MAX_D):
        raise ValueError(f"ideal: the feature width {d} must be a multiple of 64 in 64..{MAX_D}")


class TrainingSet:
    """A training set prepared for the ideal denoiser: ``FeatureSet``'s planes and norms, the planes transposed ([3, d, Np], pad columns zero) and the fp32
    rows themselves (``feats``: what ``x0`` is a convex combination of).  ``feats``: fp32 [N, d] or a ``FeatureSet`` (then ``feats`` is its hi + mid + lo)."""

    def __init__(self, feats, device=None):
        L = _lib()
        if isinstance(feats, FeatureSet):
            self.set = feats
            self.feats = feats.planes.float().sum(0)            # (hi + mid) + lo, both sums exact
        else:
            feats = torch.as_tensor(feats)
            if feats.dim() != 2 or feats.dtype != torch.float32:
                raise ValueError(f"ideal: a training set must be an fp32 [N, d] tensor, got {feats.dtype} {tuple(feats.shape)}")
            check_width(int(feats.shape[1]))
            self.set = FeatureSet(feats, device=device)
            self.feats = feats.to(self.set.device).contiguous()
        self.n, self.d, self.device = self.set.n, self.set.d, self.set.device
        check_width(self.d)
        self.planes, self.norms = self.set.planes, self.set.norms
        self.tplanes = torch.empty(3, self.d, padded_cols(self.n), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib.natinf_ideal_tplanes(L.ptr(self.planes), self.n, self.d, L.ptr(self.tplanes), L.stream_ptr()), "natinf_ideal_tplanes")


def level_scalars(x_t, alpha, sigma):
    """(u, c) of a noise level: u = fp32(x_t / alpha) evaluated in fp64 and c = alpha^2 / (2 sigma^2) in fp64.  ``alpha`` / ``sigma``: scalars or one
    value per row of ``x_t`` ([B, ...]; host numbers or arrays, or fp64 tensors on ``x_t``'s device), sigma > 0 and alpha != 0.  ``c`` comes back as a
    numpy fp64 [B] for host levels and as an fp64 tensor for device ones."""
    x_t = torch.as_tensor(x_t)
    if x_t.dtype != torch.float32 or x_t.dim() < 2:
        raise ValueError(f"ideal: x_t must be fp32 [B, ...], got {x_t.dtype} {tuple(x_t.shape)}")
    B = int(x_t.shape[0])
    if isinstance(alpha, torch.Tensor) or isinstance(sigma, torch.Tensor):
        a = torch.as_tensor(alpha, dtype=torch.float64, device=x_t.device).expand(B)
        s = torch.as_tensor(sigma, dtype=torch.float64, device=x_t.device).expand(B)
        c = a * a / (2.0 * s * s)
    else:
        a_np = np.broadcast_to(np.asarray(alpha, np.float64), (B,))
        s_np = np.broadcast_to(np.asarray(sigma, np.float64), (B,))
        if not (np.isfinite(a_np).all() and np.isfinite(s_np).all() and (s_np > 0).all() and (a_np != 0).all()):
            raise ValueError("ideal: a level needs finite alpha != 0 and sigma > 0")
        c = a_np * a_np / (2.0 * s_np * s_np)
        a = torch.from_numpy(np.array(a_np)).to(x_t.device)
    u = (x_t.double() / a.reshape((B,) + (1,) * (x_t.dim() - 1))).float()
    return u, c


def _row_scalars(v, n: int, device, name: str, positive: bool = False) -> torch.Tensor:
    """fp64 [n] on the device.  Host data (a number, a sequence, an array, a CPU tensor) is checked here: finite, and >= 0 (``c``) or > 0 (``sigma``);
    a device tensor is not read back (include/natinf_ideal.h states what other values give)."""
    if isinstance(v, torch.Tensor) and v.is_cuda:
        if v.dtype != torch.float64 or tuple(v.shape) != (n,):
            raise ValueError(f"ideal: {name} on the device must be fp64 [{n}], got {v.dtype} {tuple(v.shape)}")
        return v.to(device).contiguous()
    a = np.asarray(v.numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(n, float(a))
    if a.shape != (n,):
        raise ValueError(f"ideal: {name} must be a number or one value per row ([{n}]), got {a.shape}")
    if not np.isfinite(a).all() or (positive and not (a > 0).all()) or (name == "c" and (a < 0).any()):
        raise ValueError(f"ideal: {name} must be finite and " + ("> 0" if positive else ">= 0" if name == "c" else "given"))
    return torch.from_numpy(np.array(a)).to(device)


def _check_rows(rows, train, what: str = "rows") -> torch.Tensor:
    rows = torch.as_tensor(rows)
    if rows.dtype != torch.float32 or rows.dim() != 2 or int(rows.shape[1]) != train.d:
        raise ValueError(f"ideal: {what} must be fp32 [B, {train.d}], got {rows.dtype} {tuple(rows.shape)}")
    if int(rows.shape[0]) > MAX_N:
        raise ValueError(f"ideal: at most {MAX_N} rows a call")
    return rows


def _workspace(L, n_rows: int, train) -> torch.Tensor:
    nbytes = L.lib.natinf_ideal_workspace_bytes(n_rows, train.n, train.d)
    L.check(min(nbytes, 0), "natinf_ideal_workspace_bytes")
    return torch.empty(nbytes, dtype=torch.uint8, device=train.device)


def posterior_mean(rows, c, train: TrainingSet, *, x=None, alpha=None, sigma=None, self_offset: int = -1, return_stats: bool = False):
    """x0 fp32 [B, d] on the device: the posterior mean of every row of ``rows`` (fp32 [B, d]) at scale ``c`` (a number or one per row, >= 0) over
    ``train``.  With ``x`` (fp32 [B, d]), ``alpha`` and ``sigma`` (numbers or one per row) the result is ``(x0, out)``, ``out`` =
    fp32((x - alpha x0_exact) / sigma): the prediction in the eps form a score network returns.  ``self_offset`` >= 0 leaves training row
    ``self_offset + i`` out of row i (a set against itself: 0).  ``return_stats`` appends dict(lse, pmax fp64 [B]; nearest int64 [B]: the lowest
    training row at the smallest distance)."""
    if not isinstance(train, TrainingSet):
        raise ValueError("ideal: train must be a TrainingSet")
    rows = _check_rows(rows, train)
    B = int(rows.shape[0])
    eps_form = x is not None
    if eps_form != (alpha is not None) or eps_form != (sigma is not None):
        raise ValueError("ideal: x, alpha and sigma come together")
    if eps_form:
        x = _check_rows(x, train, "x")
        if int(x.shape[0]) != B:
            raise ValueError("ideal: x and rows differ in their number of rows")
    if self_offset < -1 or (self_offset >= 0 and self_offset + B > train.n):
        raise ValueError("ideal: self_offset must be -1 or an offset that keeps every left-out row inside the training set")
    if train.n < 1 + (self_offset >= 0):
        raise ValueError("ideal: the training set is too small to leave a row out")
    dev = train.device
    c_t = _row_scalars(c, B, dev, "c")
    a_t = _row_scalars(alpha, B, dev, "alpha") if eps_form else None
    s_t = _row_scalars(sigma, B, dev, "sigma", positive=True) if eps_form else None
    L = _lib()
    rows = rows.to(dev).contiguous()
    x = x.to(dev).contiguous() if eps_form else None
    x0 = torch.empty(B, train.d, dtype=torch.float32, device=dev)
    out = torch.empty_like(x0) if eps_form else None
    lse = torch.empty(B, dtype=torch.float64, device=dev) if return_stats else None
    pmax = torch.empty(B, dtype=torch.float64, device=dev) if return_stats else None
    near = torch.empty(B, dtype=torch.int32, device=dev) if return_stats else None
    if B:
        ws = _workspace(L, B, train)
        with torch.cuda.device(dev):
            L.check(L.lib.natinf_ideal_posterior_mean(L.ptr(rows), L.ptr(c_t), B, L.ptr(train.planes), L.ptr(train.norms), L.ptr(train.tplanes), train.n,
                                                      train.d, self_offset, L.ptr(x), L.ptr(a_t), L.ptr(s_t), L.ptr(x0), L.ptr(lse), L.ptr(pmax),
                                                      L.ptr(near), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr()), "natinf_ideal_posterior_mean")
    res = (x0, out) if eps_form else (x0,)
    if return_stats:
        res += (dict(lse=lse, pmax=pmax, nearest=near.long()),)
    return res[0] if len(res) == 1 else res


def debug_weights(rows, c, train: TrainingSet, self_offset: int = -1):
    """(w fp32 [B, N], planes bf16 [3, B, Np]) -- the staged weights and the planes they are the sum of (test hook; B N <= 2^20)"""
    L = _lib()
    rows = _check_rows(rows, train).to(train.device).contiguous()
    B = int(rows.shape[0])
    c_t = _row_scalars(c, B, train.device, "c")
    w = torch.empty(B, train.n, dtype=torch.float32, device=train.device)
    planes = torch.empty(3, B, padded_cols(train.n), dtype=torch.bfloat16, device=train.device)
    ws = _workspace(L, B, train)
    with torch.cuda.device(train.device):
        L.check(L.lib.natinf_ideal_debug_weights(L.ptr(rows), L.ptr(c_t), B, L.ptr(train.planes), L.ptr(train.norms), train.n, train.d, self_offset,
                                                 L.ptr(w), L.ptr(planes), L.ptr(ws), ws.numel(), L.stream_ptr()), "natinf_ideal_debug_weights")
    return w, planes


def levels_of_labels(labels):
    """(alpha, sigma) fp64 arrays of the VP levels a CIFAR10 job's ``labels`` (t * 999) name: t = labels / 999 in fp64, ``coeffgen.vp_alpha_sigma``."""
    from .coeffgen import vp_alpha_sigma
    lab = np.asarray(labels.detach().cpu() if isinstance(labels, torch.Tensor) else labels, dtype=np.float64).reshape(-1)
    return vp_alpha_sigma(lab / 999.0)


def train_images_to_feats(train_images) -> torch.Tensor:
    """uint8 [N, 32, 32, 3] pixels (through ``u8_to_centered``) or centred fp32 [N, 3, 32, 32] -> fp32 [N, 3072] in the NCHW order a ``model_fn`` sees"""
    t = torch.as_tensor(train_images)
    if t.dtype == torch.uint8 and t.dim() == 4 and tuple(t.shape[1:]) == (32, 32, 3):
        t = ((t.permute(0, 3, 1, 2).to(torch.float64) + 0.5) / 255.0 * 2.0 - 1.0).to(torch.float32)       # u8_to_centered
    elif not (t.dtype == torch.float32 and t.dim() == 4 and tuple(t.shape[1:]) == (3, 32, 32)):
        raise ValueError(f"ideal: train_images must be uint8 [N, 32, 32, 3] or centred fp32 [N, 3, 32, 32], got {t.dtype} {tuple(t.shape)}")
    return t.reshape(t.shape[0], -1).contiguous()


class IdealDenoiser:
    """The ideal denoiser of a CIFAR10-shaped training set as a ``model_fn``: ``denoiser(x [B, 3, 32, 32], labels [B])`` reads t = labels / 999, takes
    alpha and sigma from ``coeffgen.vp_alpha_sigma`` in fp64 and returns ``out`` = (x - alpha E[x0 | x]) / sigma, from which the fused step recovers the
    posterior mean.  A drop-in for ``CifarNI.run``, ``natural_inference`` and ``generate_sharded`` (a plain callable: one lane); every image of such a
    job collapses onto a training image.  ``train_images``: see ``train_images_to_feats``, or a ``TrainingSet`` of width 3,072.  Reading the labels
    waits for the stream once per call."""

    def __init__(self, train_images, device=None):
        self.train = train_images if isinstance(train_images, TrainingSet) else TrainingSet(train_images_to_feats(train_images), device=device)
        if self.train.d != 3 * 32 * 32:
            raise ValueError("ideal: an IdealDenoiser's training set holds 3 x 32 x 32 images")
        self.device = self.train.device

    def x0(self, x: torch.Tensor, labels, return_stats: bool = False):
        """The posterior mean itself, [B, 3, 32, 32] (and the statistics of ``posterior_mean``)"""
        res = self._run(x, labels, return_stats)
        return (res[0].view(x.shape),) + tuple(res[2:]) if return_stats else res[0].view(x.shape)

    def _run(self, x, labels, return_stats=False):
        if x.dtype != torch.float32 or x.dim() != 4 or tuple(x.shape[1:]) != (3, 32, 32):
            raise ValueError(f"ideal: x must be fp32 [B, 3, 32, 32], got {x.dtype} {tuple(x.shape)}")
        alpha, sigma = levels_of_labels(labels)
        if alpha.shape != (x.shape[0],):
            raise ValueError("ideal: one label per image")
        flat = x.reshape(x.shape[0], -1)
        u, c = level_scalars(flat, alpha, sigma)
        return posterior_mean(u, c, self.train, x=flat, alpha=alpha, sigma=sigma, return_stats=return_stats)

    def __call__(self, x: torch.Tensor, labels) -> torch.Tensor:
        return self._run(x, labels)[1].view(x.shape)
