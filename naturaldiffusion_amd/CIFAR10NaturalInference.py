"""Drop-in for ``src/CIFAR10NaturalInference.py`` (the Natural Inference part, lines 202-317).

Same public names, argument meaning and defaults as the reference script: ``to_pixel``, ``data_fn``,
``weighted_sum``, ``natural_inference_tx``, ``calc_fid``.  The sampling loop runs on one MI355X:
the NCSN++ forward in the HIP engine (include/natinf_ncsnpp.h) and one fused ``ni_step`` launch per
step (include/natinf.h).  Constants the reference edits in-source are keyword arguments with the
reference's values as defaults (batch 500, 50 000 samples, seed 888, step_5_weight_00.npz).
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ptr, stream_ptr
from .coeff import load_coeff_npz, SparseRows
from .jobs import KnownRows, check_row_count, gather_known, host_mask, mask_table  # noqa: F401  (gather_known: importable from here as before)
from .sampler import CifarNI, check_project, check_x0_fix, decouple0_host, downsample_host, vp_std_f32

root_path = Path(__file__).resolve().parent.parent


def _to_pixel(x: torch.Tensor, centered: int, to_cpu: bool = True) -> torch.Tensor:
    _lib.require_gpu()
    x = x.contiguous()
    B, C, H, W = x.shape
    out = torch.empty((B, H, W, C), dtype=torch.uint8, device=x.device)
    check(lib.natinf_to_pixel_u8(ptr(x), ptr(out), B, C, H, W, centered, stream_ptr()), "natinf_to_pixel_u8")
    return out.cpu() if to_cpu else out            # (the copy to the host blocks: the batch pipeline of natural_inference_tx copies at the end)


def to_pixel(batch: torch.Tensor) -> torch.Tensor:
    """Reference :212-216: [B,C,H,W] fp32 in [0,1] -> uint8 [B,H,W,C] on the CPU."""
    return _to_pixel(batch, 0)


def to_pixel_from_centered(x: torch.Tensor) -> torch.Tensor:
    """inverse_scaler (datasets.py:32-38) + to_pixel in one launch: x in [-1,1] -> uint8 NHWC (CPU)."""
    return _to_pixel(x, 1)


@torch.no_grad()
def data_fn(score_fn: Callable, xt: torch.Tensor, t, x_coeff, eps_coeff, device) -> torch.Tensor:
    """Reference :219-230.  ``score_fn(xt, vec_t)`` is the caller's score function; the fp64 conversion
    ``(score*eps_coeff**2 + xt)/x_coeff`` runs in ``natinf_step_f64hist`` (std = -1 makes its internal
    ``-out/std`` the identity on the score)."""
    _lib.require_gpu()
    vec_t = t * torch.ones(xt.shape[0], device=device)
    score = score_fn(xt, vec_t).contiguous()
    xt = xt.contiguous()
    E = xt.numel()
    hist = torch.empty((1, E), dtype=torch.float64, device=xt.device)
    scratch = torch.empty(E, dtype=torch.float32, device=xt.device)
    check(lib.natinf_step_f64hist(ptr(xt), ptr(score), ptr(xt), ptr(hist), ptr(scratch), None, None, 0, 0.0, 0,
                                  float(x_coeff), float(eps_coeff), -1.0, 0.0, E, stream_ptr()), "natinf_step_f64hist")
    return hist.view(xt.shape)


def weighted_sum(past_x0_coeff: Sequence[float], seq_x0: Sequence[torch.Tensor]) -> torch.Tensor:
    """Reference :233-238: fp64 sum_i seq_x0[i]*coeff[i] (ascending i) -> fp32."""
    _lib.require_gpu()
    slab = torch.stack([s.contiguous().reshape(-1) for s in seq_x0]).to(torch.float64)
    n, E = slab.shape
    rows = SparseRows(np.asarray(past_x0_coeff, np.float64)[None, :n], lambda k: n, torch.float64, slab.device,
                      dense=True, diag=False)
    out = torch.empty(E, dtype=torch.float32, device=slab.device)
    idx, val, nt = rows.ptrs(0)
    check(lib.natinf_weighted_sum_f64(ptr(slab), ptr(out), idx, val, nt, E, stream_ptr()), "natinf_weighted_sum_f64")
    return out.view(seq_x0[0].shape)


@torch.no_grad()
def natural_inference(model_fn: Callable, noise: torch.Tensor, weight_path, dense: bool = False,
                      fast_f32: bool = False, return_all: bool = False, stds=None, seed: int = 888, first_index: int = 0):
    """The loop body of ``natural_inference_tx`` (:292-304) for one batch of initial noise.  A stochastic matrix
    (``coeff.is_stochastic``) also injects the noise of every later column of B: image i of the batch draws column j >= 1
    from Philox(``seed``, global index ``first_index + i``, j) -- ``philox_noise(..., column=j)``."""
    C, B, node = load_coeff_npz(weight_path)
    ni = CifarNI(C, B, node, noise.numel(), device=noise.device, dense=dense, fast_f32=fast_f32, stds=stds, seed=seed)
    return ni.run(model_fn, noise, return_all=return_all, index=int(first_index))


def philox_noise(indices, shape_per_image, seed: int, device="cuda:0", column: int = 0) -> torch.Tensor:
    """[len(indices), *shape_per_image] fp32 N(0,1), image i keyed by its GLOBAL index (include/natinf.h,
    natinf_randn_philox_col_f32): identical for any GPU count / batch split.  ``column`` j >= 1 gives the noise a
    stochastic matrix injects after step j-1 (what the fused CIFAR10 step generates for column j of B)."""
    _lib.require_gpu()
    idx = torch.as_tensor(list(indices), dtype=torch.int64, device=device)
    per = int(np.prod(shape_per_image))
    out = torch.empty((idx.numel(),) + tuple(shape_per_image), dtype=torch.float32, device=device)
    check(lib.natinf_randn_philox_col_f32(ptr(out), idx.numel(), per, ptr(idx), 0, 0, int(seed) & (2 ** 64 - 1), int(column),
                                          stream_ptr()), "natinf_randn_philox_col_f32")
    return out


def u8_to_centered(v) -> torch.Tensor:
    """uint8 pixel values -> the centred fp32 value at the middle of the pixel's bin, fp32((v + 0.5)/255*2 - 1) evaluated in fp64: all 256
    values come back exactly through ``to_pixel_from_centered`` (trunc((x+1)/2*255) sits half a level from either neighbour; v/255*2 - 1, the
    bin's lower edge, would fall to v - 1 on a last-bit rounding).  255 maps to 1 + 1/255 and comes back through the clamp."""
    v = torch.as_tensor(v)
    return ((v.to(torch.float64) + 0.5) / 255.0 * 2.0 - 1.0).to(torch.float32)


def prepare_known(known, mask, sample_count: int, known_final: str = "mean"):
    """The inpainting arguments of ``generate_sharded`` -> (known fp32 [K, 3072] centred NCHW, mask uint8 [K', 3072]) on the CPU, K and K'
    each ``sample_count`` (row i belongs to global image index i) or 1 (shared by every image).  ``known``: uint8 [K, 32, 32, 3] (the job's own
    output format, mapped by ``u8_to_centered``) or fp32 [K, 3, 32, 32] centred.  ``mask``: bool / uint8 [K', 32, 32] (a pixel: broadcast over
    the channels) or [K', 3, 32, 32]; non-zero = known.  Pure host code: every refusal comes before any GPU call."""
    if known is None or mask is None:
        raise ValueError("inpainting needs both known= and mask=")
    if known_final not in ("mean", "data"):
        raise ValueError('known_final must be "mean" or "data"')
    known = torch.as_tensor(known).cpu()
    if known.dtype == torch.uint8 and known.dim() == 4 and tuple(known.shape[1:]) == (32, 32, 3):
        kf = u8_to_centered(known.permute(0, 3, 1, 2))
    elif known.dtype == torch.float32 and known.dim() == 4 and tuple(known.shape[1:]) == (3, 32, 32):
        kf = known
    else:
        raise ValueError("known must be uint8 [K, 32, 32, 3] or fp32 [K, 3, 32, 32] (centred)")
    table = mask_table(host_mask(mask), 3, 32, sample_count, forms=("element", "cell"))      # a pixel of the picture is a cell of its three planes
    if table is None:
        raise ValueError("mask must be [K, 32, 32] or [K, 3, 32, 32]")
    check_row_count("known", kf, sample_count)
    return kf.reshape(kf.shape[0], -1).contiguous(), table


def prepare_gray(gray, sample_count: int, known_final: str = "mean") -> torch.Tensor:
    """The colorization argument of ``generate_sharded`` -> gray_u fp32 [K, 1024] on the CPU: latent channel 0 (``sampler.decouple0_host``) of the
    known pictures, K ``sample_count`` (row i belongs to global image index i) or 1 (shared by every image).  ``gray``: uint8 [K, 32, 32] (a gray
    picture, taken as (g, g, g)), uint8 [K, 32, 32, 3] or fp32 [K, 3, 32, 32] centred (of a colour picture its gray channel is taken).  uint8
    values go through ``u8_to_centered``.  Pure host code: every refusal comes before any GPU call."""
    if known_final not in ("mean", "data"):
        raise ValueError('known_final must be "mean" or "data"')
    gray = torch.as_tensor(gray).cpu()
    if gray.dtype == torch.uint8 and gray.dim() == 3 and tuple(gray.shape[1:]) == (32, 32):
        gf = u8_to_centered(gray)[:, None].expand(-1, 3, -1, -1)
    elif gray.dtype == torch.uint8 and gray.dim() == 4 and tuple(gray.shape[1:]) == (32, 32, 3):
        gf = u8_to_centered(gray.permute(0, 3, 1, 2))
    elif gray.dtype == torch.float32 and gray.dim() == 4 and tuple(gray.shape[1:]) == (3, 32, 32):
        gf = gray
    else:
        raise ValueError("gray must be uint8 [K, 32, 32], uint8 [K, 32, 32, 3] or fp32 [K, 3, 32, 32] (centred)")
    check_row_count("gray", gf, sample_count)
    return torch.from_numpy(np.ascontiguousarray(decouple0_host(gf.contiguous().numpy()))).reshape(gf.shape[0], -1)


IMAGE_SHAPE = (3, 32, 32)


def _check_sr_job(lowres, sr_scale, sr_final: str, *, seed, x0_fix=None, conditioned: bool = False) -> int:
    """The super-resolution arguments of a job, checked on the host -> the scale (0: off).  ``lowres`` and ``sr_scale`` come together."""
    if sr_final not in ("step", "x0"):
        raise ValueError('sr_final must be "step" or "x0"')
    if (lowres is None) != (sr_scale is None):
        raise ValueError("super-resolution needs both lowres= and sr_scale=")
    if sr_scale is None and sr_final != "step":
        raise ValueError('sr_final="x0" belongs to super-resolution (lowres= and sr_scale=)')
    return check_project(sr_scale, IMAGE_SHAPE, seed=seed, elems_per_image=3 * 32 * 32, x0_fix=x0_fix, conditioned=conditioned)


def downsample_images(images, sr_scale: int) -> torch.Tensor:
    """The low-resolution rows of pictures -> fp64 [K, 3*(32/s)^2] on the CPU, the s x s block averages in ``sampler.downsample_host``'s order: how a
    caller (or a test) makes ``lowres`` from a picture.  ``images``: uint8 [K, 32, 32, 3] (mapped by ``u8_to_centered``) or centred fp32 [K, 3, 32, 32]."""
    images = torch.as_tensor(images).cpu()
    if images.dtype == torch.uint8 and images.dim() == 4 and tuple(images.shape[1:]) == (32, 32, 3):
        f = u8_to_centered(images.permute(0, 3, 1, 2))
    elif images.dtype == torch.float32 and images.dim() == 4 and tuple(images.shape[1:]) == (3, 32, 32):
        f = images
    else:
        raise ValueError("images must be uint8 [K, 32, 32, 3] or fp32 [K, 3, 32, 32] (centred)")
    low = downsample_host(f.contiguous().numpy().reshape(f.shape[0], -1), IMAGE_SHAPE, sr_scale)
    return torch.from_numpy(np.ascontiguousarray(low))


def prepare_lowres(lowres, sr_scale: int, sample_count: int) -> torch.Tensor:
    """The super-resolution argument of ``generate_sharded`` -> fp64 [K, 3*(32/s)^2] on the CPU, K ``sample_count`` (row i belongs to global image index
    i) or 1 (shared by every image).  ``lowres``: uint8 [K, 32/s, 32/s, 3] (mapped by ``u8_to_centered``) or fp32 / fp64 [K, 3, 32/s, 32/s] centred
    (``downsample_images`` of a picture, reshaped, is one).  Pure host code: every refusal comes before any GPU call."""
    s = check_project(sr_scale, IMAGE_SHAPE, elems_per_image=3 * 32 * 32)
    if lowres is None or not s:
        raise ValueError("super-resolution needs both lowres= and sr_scale=")
    n = 32 // s
    lowres = torch.as_tensor(lowres).cpu()
    if lowres.dtype == torch.uint8 and lowres.dim() == 4 and tuple(lowres.shape[1:]) == (n, n, 3):
        lf = u8_to_centered(lowres.permute(0, 3, 1, 2)).to(torch.float64)
    elif lowres.dtype in (torch.float32, torch.float64) and lowres.dim() == 4 and tuple(lowres.shape[1:]) == (3, n, n):
        lf = lowres.to(torch.float64)
    else:
        raise ValueError(f"lowres must be uint8 [K, {n}, {n}, 3] or fp32 / fp64 [K, 3, {n}, {n}] (centred)")
    check_row_count("lowres", lf, sample_count)
    return lf.reshape(lf.shape[0], -1).contiguous()


class BatchLanes:
    """The batch pipeline of ``natural_inference_tx`` / ``generate_sharded``: the batches of a generation job are independent
    trajectories (reference loop :287-309), so consecutive batches go to ``len(models)`` lanes -- one HIP stream, one denoiser handle and
    one set of history slabs each -- and the under-occupied launches of one batch run under the other's convolutions.
    A batch is enqueued end to end (noise, 15-18 forwards + ni_step launches, ``to_pixel``) without the host waiting for the GPU; the uint8
    images stay on the device until ``finish``; at most ``depth`` batches per lane are enqueued ahead of the GPU.  ``seed`` keys the noise a
    stochastic matrix injects after each step (``CifarNI``), per image by the global indices ``submit`` gets.  ``x0_fix`` / ``x0_ratio`` /
    ``x0_max``: the x0 correction every lane's sampler applies (``CifarNI``: "clip" or "dynamic" thresholding of each step's predicted x0);
    a bad value is a ValueError before any GPU call.  ``sr_scale``: super-resolution (``CifarNI``: every step's predicted x0 projected onto the
    low-resolution picture ``submit`` gets as ``low``); refused together with ``x0_fix``, likewise on the host."""

    def __init__(self, models, C, B, node, device, depth: int = 2, seed: Optional[int] = None,
                 x0_fix: Optional[str] = None, x0_ratio: float = 0.995, x0_max: float = 1.0, sr_scale: Optional[int] = None):
        check_x0_fix(x0_fix, x0_ratio, x0_max, seed=seed, elems_per_image=3 * 32 * 32)
        check_project(sr_scale, IMAGE_SHAPE, seed=seed, elems_per_image=3 * 32 * 32, x0_fix=x0_fix)
        self.x0 = dict(x0_fix=x0_fix, x0_ratio=x0_ratio, x0_max=x0_max) if x0_fix is not None else {}
        self.sr = dict(sr_scale=sr_scale, image_shape=IMAGE_SHAPE) if sr_scale is not None else {}
        _lib.require_gpu()
        self.device = torch.device(device)
        self.coeff = (C, B, node)
        self.models = list(models)
        multi = len(self.models) > 1
        self.streams = [torch.cuda.Stream(device=self.device) if multi else None for _ in self.models]
        self.samplers = [dict() for _ in self.models]                   # per lane: batch size -> CifarNI (a ragged last batch gets its own slabs)
        self.pending = [[] for _ in self.models]
        self.depth = int(depth)
        self.seed = seed
        self.count = 0
        self.out = []
        self.joined = [False] * len(self.models)                       # lane k has been ordered behind the caller's stream

    def _sampler(self, k: int, n: int) -> CifarNI:
        if n not in self.samplers[k]:
            self.samplers[k][n] = CifarNI(*self.coeff, n * 3 * 32 * 32, device=self.device, seed=self.seed, elems_per_image=3 * 32 * 32, **self.x0, **self.sr)
        return self.samplers[k][n]

    def submit(self, n: int, noise=None, noise_fn=None, index=None, known=None, mask=None, known_final: str = "mean", gray_u=None,
               low=None, sr_final: str = "step") -> torch.Tensor:
        """One batch of ``n`` images: ``noise`` (drawn on the CALLER's current stream) or ``noise_fn()`` (called on the lane's stream).
        ``index``: the images' global indices, which key the noise a stochastic matrix injects -- an int64 device tensor made on the
        caller's stream, the int index of the first image, or ``(first, stride)`` (``CifarNI.step``).  ``known`` / ``mask`` (inpainting): device
        tensors made on the caller's stream, forwarded to ``CifarNI.run``; ``gray_u`` (colorization) likewise; ``low`` / ``sr_final`` (super-resolution, lanes made with
        ``sr_scale``) likewise.  Returns the uint8 [n, 32, 32, 3] DEVICE tensor the lane will fill."""
        idx_t = isinstance(index, torch.Tensor)
        if gray_u is not None and self.x0:
            raise ValueError("x0_fix does not go with gray_u (colorization)")
        if sr_final not in ("step", "x0"):
            raise ValueError('sr_final must be "step" or "x0"')
        if self.sr:
            check_project(self.sr["sr_scale"], IMAGE_SHAPE, seed=self.seed, elems_per_image=3 * 32 * 32,
                          conditioned=known is not None or mask is not None or gray_u is not None)
            if low is None:
                raise ValueError("lanes made with sr_scale need low= for every batch")
        elif low is not None or sr_final != "step":
            raise ValueError('low= and sr_final="x0" belong to lanes made with sr_scale')
        inpaint = [t for t in (known, mask, gray_u, low) if t is not None]  # the lane is ordered behind their upload
        k = self.count % len(self.models)
        self.count += 1
        st = self.streams[k]
        if len(self.pending[k]) >= self.depth:                          # bound the host's run-ahead (and the noise tensors in flight)
            self.pending[k].pop(0).synchronize()
        with torch.cuda.device(self.device):
            # A lane's first launch is ordered behind everything the caller's stream has queued: the engine's workspace and packed weights (and
            # the blocks clone() got from the caching allocator, which may be recycled ones with work pending) were allocated THERE, and a
            # still-queued forward of lane 0's engine on the caller's stream would otherwise race with the lane's.  With `noise` every submit waits.
            if st is not None and (noise is not None or idx_t or inpaint or not self.joined[k]):
                st.wait_stream(torch.cuda.current_stream())
                self.joined[k] = True
            if st is not None and noise is not None:
                noise.record_stream(st)
            if st is not None and idx_t:
                index.record_stream(st)
            if st is not None:
                for t in inpaint:
                    t.record_stream(st)
            with torch.cuda.stream(st):
                ni = self._sampler(k, n)                                # (first use allocates on the lane's stream)
                z = noise if noise is not None else noise_fn()
                kw = dict(known=known, mask=mask, known_final=known_final) if known is not None or mask is not None else {}
                if gray_u is not None:
                    kw.update(gray_u=gray_u, known_final=known_final)
                if self.sr:
                    kw.update(low=low, sr_final=sr_final)
                pix = _to_pixel(ni.run(self.models[k], z, index=index, **kw), 1, to_cpu=False)
                ev = torch.cuda.Event()
                ev.record()
        self.pending[k].append(ev)
        self.out.append(pix)
        return pix

    def finish(self):
        """Wait for every lane (the caller's stream then sees the images); returns the list of per-batch uint8 device tensors."""
        with torch.cuda.device(self.device):
            main = torch.cuda.current_stream()
            for st in self.streams:
                if st is not None:
                    main.wait_stream(st)
            if any(st is not None for st in self.streams):
                for pix in self.out:                                     # allocated on a lane's stream, consumed (and freed) on the caller's: the allocator must
                    pix.record_stream(main)                              # not hand the block back to the lane while the caller's torch.cat is still queued
        self.pending = [[] for _ in self.models]
        self.joined = [False] * len(self.models)
        out, self.out = self.out, []
        return out


def _lane_models(model_fn, streams: int, n_batches: int):
    """One denoiser per lane.  An ``NCSNppEngine`` is cloned (own launch plan + workspace, shared packed weights); a sequence of callables
    is taken as given (one lane each); any other callable owns state we cannot duplicate, so it gets one lane."""
    from .ncsnpp import NCSNppEngine
    if isinstance(model_fn, (list, tuple)):
        return list(model_fn)
    n = max(1, min(int(streams), n_batches))
    if isinstance(model_fn, NCSNppEngine):
        return [model_fn] + [model_fn.clone() for _ in range(n - 1)]
    return [model_fn]


@torch.no_grad()
def generate_sharded(model_fn, weight_path, sample_count: int, batch_size: int, rank: int = 0, world: int = 1,
                     seed: int = 888, device="cuda:0", streams: int = 3, to_cpu: bool = True, coeff=None,
                     known=None, mask=None, known_final: str = "mean", gray=None,
                     x0_fix: Optional[str] = None, x0_ratio: float = 0.995, x0_max: float = 1.0,
                     lowres=None, sr_scale: Optional[int] = None, sr_final: str = "step"):
    """Batch-sharded generation (BASELINE config 3): this rank generates the images whose
    global index is rank, rank+world, ... in batches of ``batch_size`` -- no collective on the data path -- on the two-lane pipeline
    of ``natural_inference_tx`` (``BatchLanes``): Philox noise keyed by the GLOBAL image index drawn on the lane's own stream, uint8 images
    kept on the device, one copy to the host at the end (none with ``to_cpu=False``: ``calc_fid_sharded`` scores device tensors).
    ``model_fn``: an ``NCSNppEngine`` (cloned per lane), a sequence of callables (one lane each) or one callable (one lane).
    ``coeff``: (C, B, node_coeff) instead of a file (matrices from ``coeffgen``).  A stochastic matrix draws the noise it injects after each
    step from the same (seed, global index) key, column j of B as counter word 3: an image's whole noise is Philox(seed, global index, column).
    ``known`` / ``mask`` (inpainting, ``prepare_known``): the pixels of image i that are given -- row i of each, or its only row -- come back as
    ``known`` at the last level (``known_final="mean"``: alpha_N * known, the reference's ``x_mean``) or exactly as given (``"data"``), and the rest
    of the image is generated around them: every step overwrites them with the data diffused to the step's level.
    ``gray`` (colorization, ``prepare_gray``): the gray picture of image i -- row i, or the only row -- comes back as the gray channel of the result
    (at the last level for ``known_final="mean"``, as given for ``"data"``) and the colours are generated around it: every step overwrites latent
    channel 0 of a rotated colour space with the gray data diffused to the step's level.  Not together with ``known`` / ``mask``.
    ``x0_fix`` (x0 correction): ``"clip"`` clamps every step's predicted x0 to [-``x0_max``, ``x0_max``] (DDPM's clip_denoised);
    ``"dynamic"`` clamps it to, and divides it by, s = max(the ``x0_ratio`` quantile of the image's |x0|, ``x0_max``) (Imagen's dynamic thresholding, the
    reference's ``correcting_x0_fn="dynamic_thresholding"``), inside the step's launch, before the history and the sum see it.  A per-image function: image
    i stays the same bytes for any split.  It goes with ``known`` / ``mask``, not with ``gray``; ``None`` (default) is the job without the option.
    ``lowres`` / ``sr_scale`` (super-resolution, ``prepare_lowres``): the low-resolution picture of image i -- row i, or the only row --
    at 1 / ``sr_scale`` (2, 4 or 8) of the size; every step projects its predicted x0 onto the pictures whose block averages are that picture, inside the
    step's launch (DDNM).  ``sr_final="step"`` returns x_N as every other job does, ``"x0"`` the last projected prediction, whose block means are the data.
    A function of the image's own x0 and its own row: image i stays the same bytes for any split.  Not together with ``known`` / ``mask``, ``gray`` or ``x0_fix``.
    Returns (uint8 images [n_local, 32, 32, 3], their global indices [n_local] int64 on the CPU)."""
    from .shard import rank_batches
    check_x0_fix(x0_fix, x0_ratio, x0_max, seed=seed, elems_per_image=3 * 32 * 32, gray=gray is not None)
    inpaint = known is not None or mask is not None
    if _check_sr_job(lowres, sr_scale, sr_final, seed=seed, x0_fix=x0_fix, conditioned=inpaint or gray is not None):
        lowres = prepare_lowres(lowres, sr_scale, sample_count)
    if gray is not None:
        if inpaint:
            raise ValueError("gray (colorization) does not go with known / mask (inpainting)")
        gray = prepare_gray(gray, sample_count, known_final)
    if inpaint:
        known, mask = prepare_known(known, mask, sample_count, known_final)
    C, B, node = coeff if coeff is not None else load_coeff_npz(weight_path)
    batches = list(rank_batches(sample_count, batch_size, rank, world))
    dev = torch.device(device)
    if not batches:
        return torch.empty((0, 32, 32, 3), dtype=torch.uint8, device="cpu" if to_cpu else dev), torch.empty(0, dtype=torch.int64)
    lanes = BatchLanes(_lane_models(model_fn, streams, len(batches)), C, B, node, dev, seed=seed, x0_fix=x0_fix, x0_ratio=x0_ratio, x0_max=x0_max,
                       sr_scale=sr_scale)
    rows = (KnownRows(dev, known=known, mask=mask) if inpaint else KnownRows(dev, gray_u=gray) if gray is not None else
            KnownRows(dev, low=lowres) if sr_scale is not None else None)
    for batch in batches:                                                # the batch's rows are uploaded here, on the caller's stream, in front of submit
        kw = dict(rows.batch(batch), sr_final=sr_final) if sr_scale is not None else dict(rows.batch(batch), known_final=known_final) if rows is not None else {}
        lanes.submit(len(batch), noise_fn=lambda b=batch: philox_noise(b, (3, 32, 32), seed, dev), index=(batch[0], world), **kw)   # = batch
    imgs = torch.cat(lanes.finish())
    idxs = torch.cat([torch.tensor(b, dtype=torch.int64) for b in batches])
    return (imgs.cpu() if to_cpu else imgs), idxs


INCEPTION_WEIGHTS = "pt_inception-2015-12-05-6726825d.pth"      # what pytorch_fid downloads on first use (FID_WEIGHTS_URL)


def inception_weights_path() -> Path:
    """$NATINF_INCEPTION_WEIGHTS, else weights/pt_inception-2015-12-05-6726825d.pth next to the coefficient files, else the torch hub
    cache pytorch_fid fills (~/.cache/torch/hub/checkpoints)."""
    env = os.environ.get("NATINF_INCEPTION_WEIGHTS")
    if env:
        return Path(env)
    for cand in (root_path / "weights" / INCEPTION_WEIGHTS, Path.home() / ".cache/torch/hub/checkpoints" / INCEPTION_WEIGHTS):
        if cand.exists():
            return cand
    return root_path / "weights" / INCEPTION_WEIGHTS


FID_BATCH = 500      # images per Inception call.  The reference feeds 50 (:47); an image's features do not depend on its batch (the same bytes at 50 and 500,
                     # tests/test_gpu_inception.py) and the engine runs 8,500 images/s in 50s, 11,400 in 500s


def _fid_batch(model) -> int:
    return max(1, min(FID_BATCH, int(getattr(model, "max_batch", 50))))


def fid_inception(device, image_hw=(32, 32), max_batch: int = FID_BATCH):
    """The pool3 network of ``calc_fid`` on the HIP library (include/natinf_inception.h) -- the reference builds
    ``InceptionV3([BLOCK_INDEX_BY_DIM[2048]])`` here (:75-77).  The weights are a download the image does not hold: without the file
    this raises (``fid: blocked``); there is no torch-module fallback."""
    from .inception import InceptionEngine, load_fid_inception_weights
    path = inception_weights_path()
    if not path.exists():
        raise FileNotFoundError(f"fid: blocked -- Inception weights {path} missing (pytorch_fid's {INCEPTION_WEIGHTS}; set NATINF_INCEPTION_WEIGHTS)")
    return InceptionEngine(load_fid_inception_weights(path), max_batch=max_batch, in_hw=image_hw, device=device)


def get_activation(imgs, model, dims: int = 2048, device=None) -> np.ndarray:
    """Reference :44-70: uint8 [n, H, W, 3] images -> pool3 activations [n, dims], ``FID_BATCH`` (or the engine's ``max_batch``) images per call
    -- the reference's 50 give the same features -- (the /255, the NCHW permutation, the 299 x 299 resize and the 2x - 1 scaling happen inside the
    engine's stem kernel)."""
    assert dims == 2048, "the HIP engine implements the pool3 (2048-dimensional) output"
    pred = np.empty((len(imgs), dims))
    bs = _fid_batch(model)
    for ii in range(0, len(imgs), bs):
        pred[ii:ii + bs] = model(imgs[ii:ii + bs]).cpu().numpy()
    return pred


def calc_fid(imgs, ref_path, device, model=None):
    """Reference :73-86 (InceptionV3 pool3 + Frechet distance).  Needs the Inception weights and the ``cifar10_mu_sigma.npz``
    statistics, neither of which ships with the reference."""
    from .fid_stats import frechet_distance
    ref = _ref_statistics(ref_path)
    on_gpu = torch.device(device).type == "cuda"
    if not on_gpu:
        ref.prefetch()                                                  # (host path: the reference covariance's square root is taken while the images go through Inception)
    model = model or fid_inception(device, tuple(imgs.shape[1:3]))
    act = get_activation(imgs, model, 2048, device)
    mu, sigma = np.mean(act, axis=0), np.cov(act, rowvar=False)
    return frechet_distance(ref, None, mu, sigma, device=device if on_gpu else None)


_REF_CACHE = {}


def _ref_statistics(ref):
    """``ref``: path of a ``cifar10_mu_sigma.npz``-style file (keys mu, sigma), a (mu, sigma) pair, or a ``fid_stats.FrechetReference`` -> a FrechetReference
    (unpacks as (mu, sigma); a file's object is kept per path and modification time, so every FID of a job shares the square root of the reference covariance)."""
    from .fid_stats import FrechetReference
    if isinstance(ref, FrechetReference):
        return ref
    if isinstance(ref, (tuple, list)):
        return FrechetReference(ref[0], ref[1])
    if not os.path.exists(ref):
        raise FileNotFoundError(f"fid: blocked -- {ref} (CIFAR10 Inception statistics) is missing")
    key = (os.path.abspath(str(ref)), os.path.getmtime(ref))
    if key not in _REF_CACHE:
        f = np.load(ref)
        _REF_CACHE.clear()
        _REF_CACHE[key] = FrechetReference(f["mu"], f["sigma"])
    return _REF_CACHE[key]


class PendingFid:
    """A Frechet distance being evaluated on a host thread (``calc_fid_sharded(..., defer=True)``): ``result()`` waits for it and returns the FID
    (None on the ranks that do not evaluate it); ``seconds`` is the thread's own wall time once it is done."""

    def __init__(self, fn):
        import threading
        self._value, self._error, self.seconds = None, None, 0.0

        def run():
            import time
            t0 = time.perf_counter()
            try:
                self._value = fn()
            except BaseException as e:                                   # surfaced by result()
                self._error = e
            self.seconds = time.perf_counter() - t0
        self._thread = threading.Thread(target=run, daemon=True)
        self._thread.start()

    def result(self):
        self._thread.join()
        if self._error is not None:
            raise self._error
        return self._value


def calc_fid_sharded(imgs, ref_path, device, group=None, model=None, timings: Optional[dict] = None, root_only: bool = False, defer: bool = False):
    """``calc_fid`` for a batch-sharded run: every rank scores ITS images (uint8 [n_local, H, W, 3], on the device or the host; ``FID_BATCH`` or the
    engine's ``max_batch`` per Inception call -- the reference's 50 give the same features), the (count, sum, outer-product sum) statistics are summed over ranks with ONE all-reduce (33.6 MB of fp64,
    fid_stats.ActivationStats) instead of gathering images or activations, and every rank returns the same FID.  ``timings`` (optional
    dict) receives the wall seconds of the three parts: inception_s, allreduce_s, frechet_s.  ``root_only``: only rank 0 evaluates the
    Frechet distance (a 2048 x 2048 matrix square root on the host: eight ranks doing it at once fight for the same cores), the others
    return None.  ``defer``: the host part (two symmetric eigen-decompositions, ~1.7 s on 8 cores; the reference side's is shared by every FID against the
    same statistics and starts when this function is entered) runs on a thread and a ``PendingFid`` is returned -- a job that scores several image sets
    (config 3 scores two coefficient matrices) generates the next set on the GPU meanwhile.  (The Inception PASS beside the next generation too -- the whole scoring
    on a thread and a HIP stream of its own -- was built and measured: both are bound by the same compute units; generation 4.67 -> 5.27 s, the job's 7.05-7.17 s
    unchanged.  Not kept.)"""
    import time
    from .fid_stats import ActivationStats, frechet_distance
    import torch.distributed as dist
    is_root = not (dist.is_available() and dist.is_initialized()) or dist.get_rank(group) == 0
    ref = _ref_statistics(ref_path)
    fdev = device if torch.device(device).type == "cuda" else None       # the Frechet distance's eigen-decompositions on the GPU (0.1 s) or, on a CPU device, on the host (1.4-2 s)
    if (is_root or not root_only) and fdev is None:
        ref.prefetch()
    model = model or fid_inception(device, tuple(imgs.shape[1:3]))
    dev = torch.device(device)
    sync = (lambda: torch.cuda.current_stream(dev).synchronize()) if dev.type == "cuda" else (lambda: None)      # (this call's stream, not the device)
    t0 = time.perf_counter()
    st = None
    bs = _fid_batch(model)
    for i in range(0, len(imgs), bs):
        a = model(imgs[i:i + bs])
        if st is None:
            st = ActivationStats(a.shape[-1], device=device)             # (pool3: 2048)
        st.update(a)
    if st is None:                                                       # a rank without images still takes part in the all-reduce
        st = ActivationStats(2048, device=device)
    sync()
    t1 = time.perf_counter()
    st.all_reduce(group)
    sync()
    t2 = time.perf_counter()
    fid = None
    if is_root or not root_only:
        mu, cov = st.mean_cov()
        if defer:
            fid = PendingFid(lambda: frechet_distance(ref, None, mu, cov, device=fdev))
        else:
            fid = frechet_distance(ref, None, mu, cov, device=fdev)
    elif defer:
        fid = PendingFid(lambda: None)
    if timings is not None:
        timings.update(inception_s=t1 - t0, allreduce_s=t2 - t1, frechet_s=time.perf_counter() - t2, images_all_ranks=int(float(st.n)))
    return fid


def get_features(imgs, model, device=None) -> torch.Tensor:
    """``get_activation`` with the pool3 features kept on the device: uint8 [n, H, W, 3] images -> fp32 [n, 2048], the same batching.  The result is on
    ``device``; with ``device=None`` it stays where the model put it (the engine's own device)."""
    bs = _fid_batch(model)
    parts = [model(imgs[ii:ii + bs]).float() for ii in range(0, len(imgs), bs)]
    if not parts:
        return torch.empty(0, 2048, dtype=torch.float32, device=device)
    feats = torch.cat(parts).contiguous()
    return feats if device is None else feats.to(device)


def _ref_features(ref_feats, device, what: str = "prdc") -> torch.Tensor:
    """``ref_feats``: an fp32-convertible [n, 2048] array / tensor or the path of a ``.npy`` holding one (the real images' pool3 features)"""
    if isinstance(ref_feats, (str, os.PathLike)):
        if not os.path.exists(ref_feats):
            raise FileNotFoundError(f"{what}: blocked -- {ref_feats} (pool3 features of the real CIFAR10 images) is missing")
        ref_feats = np.load(ref_feats)
    return torch.as_tensor(ref_feats).to(device=device, dtype=torch.float32)


def _gather_features(feats: torch.Tensor, device, group=None) -> torch.Tensor:
    """The ranks' ragged shares of feature rows, all-gathered in rank order onto ``device`` (this rank's own rows when there is no group of two or more)"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
        return feats
    world, host = dist.get_world_size(group), dist.get_backend(group) != "nccl"
    n = torch.tensor([feats.shape[0]], dtype=torch.int64, device="cpu" if host else feats.device)
    ns = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(ns, n, group=group)
    m = max(int(v) for v in ns)
    pad = torch.zeros(m, feats.shape[1], dtype=torch.float32, device=n.device)
    pad[:feats.shape[0]] = feats
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    return torch.cat([p[:int(c)] for p, c in zip(parts, ns)]).to(device)


def calc_prdc(imgs, ref_feats, device, model=None, k: int = 3) -> dict:
    """dict(precision, recall, density, coverage) of the images (uint8 [n, H, W, 3]) against the real images' pool3 features ``ref_feats`` (array or ``.npy``
    path): k-nearest-neighbour manifold metrics on the features ``calc_fid`` is computed from (prdc.py; include/natinf_prdc.h).  The real CIFAR10 features
    are a download the image does not hold, like FID's statistics: a missing file raises ``prdc: blocked``."""
    from . import prdc as P
    real = _ref_features(ref_feats, device)
    model = model or fid_inception(device, tuple(imgs.shape[1:3]))
    counts = P.prdc_counts(P.FeatureSet(real, device=device), P.FeatureSet(get_features(imgs, model, device), device=device), k)
    return P.prdc_from_sums(P.count_sums(counts), k)                    # this process's images only, whatever process group exists


def calc_prdc_sharded(imgs, ref_feats, device, group=None, model=None, k: int = 3) -> dict:
    """``calc_prdc`` for a batch-sharded run: every rank scores ITS images, the features (8 KB per image) are all-gathered so that every rank holds the whole
    generated set as columns, each rank measures its row slice of both sets and one all-reduce of six integers gives every rank the same four numbers."""
    import torch.distributed as dist
    from . import prdc as P
    real = _ref_features(ref_feats, device)
    model = model or fid_inception(device, tuple(imgs.shape[1:3]))
    feats = _gather_features(get_features(imgs, model, device), device, group)
    return P.prdc(P.FeatureSet(real, device=device), P.FeatureSet(feats, device=device), k=k, group=group)


def _nearest_table(imgs, ref, device, space: str, k: int, model):
    """(d2 fp64 [n, k], idx int64 [n, k]) on the device: this process's images against the whole reference"""
    from . import neighbours as N
    from .prdc import FeatureSet
    if space == "pixel":
        ref = torch.as_tensor(ref)
        if tuple(ref.shape[1:]) != tuple(imgs.shape[1:]):
            raise ValueError(f"nearest: the reference images {tuple(ref.shape[1:])} and the generated ones {tuple(imgs.shape[1:])} differ in shape")
        cols, rows = N.pixel_features(ref, device), N.pixel_features(imgs, device)
    elif space == "pool3":
        cols = _ref_features(ref, device, "nearest")
        model = model or fid_inception(device, tuple(imgs.shape[1:3]))
        rows = get_features(imgs, model, device)
    else:
        raise ValueError(f"nearest: space must be 'pixel' or 'pool3', got {space!r}")
    return N.nearest(FeatureSet(rows, device=device), FeatureSet(cols, device=device), k=k)


def _gather_rows_of(t: torch.Tensor, group) -> torch.Tensor:
    """The ranks' ragged shares of rows of a 2-d tensor, all-gathered in rank order (``_gather_features``'s scheme for any dtype; the result stays on ``t``'s device)"""
    import torch.distributed as dist
    world, host = dist.get_world_size(group), dist.get_backend(group) != "nccl"
    n = torch.tensor([t.shape[0]], dtype=torch.int64, device="cpu" if host else t.device)
    ns = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(ns, n, group=group)
    pad = torch.zeros(max(int(v) for v in ns), t.shape[1], dtype=t.dtype, device=n.device)
    pad[:t.shape[0]] = t
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    return torch.cat([p[:int(c)] for p, c in zip(parts, ns)]).to(t.device)


def _nearest_result(d2: torch.Tensor, idx: torch.Tensor, space: str, k: int) -> dict:
    from . import neighbours as N
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    return dict(d2=d2, idx=idx, summary=N.summary(d2), space=space, k=k)


def calc_nearest(imgs, ref, device, space: str = "pixel", k: int = 1, model=None) -> dict:
    """The memorisation audit beside the FID table: for every image (uint8 [n, H, W, 3]) its ``k`` nearest reference images.  dict(d2 fp64 [n, k],
    idx int64 [n, k] -- host arrays, nearest first, among equal distances the lower reference index first --, summary: ``neighbours.summary``'s min /
    median / mean of the nearest distance and the count of exact copies, space, k).  ``space="pixel"``: ``ref`` is the training images as uint8
    [M, H, W, 3] and d2 is the exact integer sum of squared pixel differences (values 0..255).  ``space="pool3"``: ``ref`` is what ``calc_prdc``
    takes as ``ref_feats`` and d2 is the squared distance of the Inception features ``calc_fid`` is computed from.  The M x n distances are never
    stored (neighbours.py; include/natinf_nn.h)."""
    d2, idx = _nearest_table(imgs, ref, device, space, k, model)
    return _nearest_result(d2, idx, space, k)                            # this process's images only, whatever process group exists


def calc_nearest_sharded(imgs, ref, device, space: str = "pixel", k: int = 1, model=None, group=None) -> dict:
    """``calc_nearest`` for a batch-sharded run: every rank measures ITS images against the whole reference (a row's neighbours depend on no other row), the
    ranks' tables are all-gathered in rank order as ``calc_prdc_sharded`` gathers features, and every rank returns the same dict: that of one process on
    rank 0's images, then rank 1's, ...  With ``group=None`` and no process group it is ``calc_nearest``."""
    import torch.distributed as dist
    d2, idx = _nearest_table(imgs, ref, device, space, k, model)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        d2, idx = _gather_rows_of(d2, group), _gather_rows_of(idx, group)
    return _nearest_result(d2, idx, space, k)


def ideal_denoiser(train_images, device="cuda:0"):
    """The ideal (empirical-Bayes) denoiser of ``train_images`` (uint8 [N, 32, 32, 3] or centred fp32 [N, 3, 32, 32]) as a ``model_fn`` for
    ``natural_inference`` / ``generate_sharded``: every step's x0 is the posterior mean over the training set, so every generated image collapses
    onto a training image -- the positive control of ``calc_nearest`` (ideal.py; include/natinf_ideal.h)."""
    from .ideal import IdealDenoiser
    return IdealDenoiser(train_images, device=device)


@torch.no_grad()
def calc_denoiser_gap(model_fn, train, ts, rows, seed: int = 888, device="cuda:0", group=None, batch_size: int = 256) -> dict:
    """How far a network's x0 prediction is from the optimal one, per noise level.  ``train``: the training images (``ideal_denoiser``'s argument), an
    ``ideal.TrainingSet`` or an ``IdealDenoiser``; ``ts``: the levels' times; ``rows``: indices of the training images that are noised, image r with
    ``philox_noise`` keyed by r (the same noise at every level), x_t = alpha f_r + sigma eps at the level the label fp32(t) * 999 names.  Both
    denoisers see (x_t, labels); both outputs become x0 = (x_t - sigma out) / alpha in fp64, so a ``model_fn`` that IS the ideal denoiser has a gap
    of exactly 0.  dict of fp64 arrays, one entry per level: ``t``; ``gap`` mean |x0_net - x0_ideal|^2 / d; ``ideal_mse`` mean |E[x0 | x_t] - f_r|^2 / d;
    ``pmax`` the mean largest posterior weight; ``own`` the share of rows whose nearest training image is their own.  In a process group every rank
    measures ``prdc.row_slice`` of ``rows`` and one all-reduce gives every rank the same dict."""
    import torch.distributed as dist
    from .ideal import IdealDenoiser, TrainingSet, levels_of_labels
    from .prdc import row_slice
    den = train if isinstance(train, IdealDenoiser) else IdealDenoiser(train, device=device)
    dev, d = den.device, den.train.d
    rows = [int(r) for r in rows]
    if not rows or min(rows) < 0 or max(rows) >= den.train.n:
        raise ValueError("denoiser gap: rows must be indices of training images")
    on = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    mine = [rows[i] for i in (row_slice(len(rows), dist.get_rank(group), dist.get_world_size(group)) if on else range(len(rows)))]
    ts = np.asarray(ts, np.float64).reshape(-1)
    sums = torch.zeros(len(ts), 4, dtype=torch.float64, device=dev)
    for b0 in range(0, len(mine), batch_size):
        batch = mine[b0:b0 + batch_size]
        f = den.train.feats[torch.as_tensor(batch, device=dev)].view(-1, 3, 32, 32)
        eps = philox_noise(batch, (3, 32, 32), seed, dev)
        for li, t in enumerate(ts):
            labels = torch.full((len(batch),), float(np.float32(t) * np.float32(999)), dtype=torch.float32, device=dev)
            alpha, sigma = (float(v[0]) for v in levels_of_labels(labels[:1]))
            x = (alpha * f.double() + sigma * eps.double()).float()
            recover = lambda out: (x.double() - sigma * out.double()) / alpha
            x0_mean, out_ideal, st = den._run(x, labels, return_stats=True)
            gap = (recover(model_fn(x, labels)) - recover(out_ideal.view(x.shape))).reshape(len(batch), -1).pow(2).sum(1) / d
            mse = (x0_mean.double() - f.reshape(len(batch), -1).double()).pow(2).sum(1) / d
            own = (st["nearest"] == torch.as_tensor(batch, device=dev)).double()
            sums[li] += torch.stack([gap.sum(), mse.sum(), st["pmax"].sum(), own.sum()])
    if on:
        host = dist.get_backend(group) != "nccl"
        sums = sums.cpu() if host else sums
        dist.all_reduce(sums, group=group)
    s = sums.cpu().numpy() / len(rows)
    return dict(t=ts, gap=s[:, 0], ideal_mse=s[:, 1], pmax=s[:, 2], own=s[:, 3])


@torch.no_grad()
def fit_coeff_matrix(model_fn, init_path, teacher, sample_count: int, out_path=None, seed: int = 888, *, holdout: Optional[int] = None,
                     device="cuda:0", **fit_kw) -> dict:
    """Fit the coefficient matrix in ``init_path`` to a teacher run (``teacher``: the path of a matrix file or a (C, B, node) triple, deterministic, with
    a node at the end of every fitted row) on ``sample_count`` images and write it to ``out_path`` (``coeffgen.save_coeff_matrix``: it loads through
    ``coeff.load_coeff_npz`` like a shipped file).  The noise of image i is ``philox_noise`` keyed by its global index i, as ``generate_sharded`` draws
    it.  ``fit_kw``: ``fit.fit_matrix``'s rows, order, ridge, constraint, batch_size, t_tol.  -> ``fit_matrix``'s report, with ``C``, ``B``, ``node``
    and, for ``holdout`` > 0 (default: ``sample_count``), ``holdout``: dict(n, indices (first, last), init_mse, fit_mse, ratio) -- the final mean
    squared difference to the teacher of the init matrix and of the fitted one on ``holdout`` images of fresh indices ``sample_count ...``: what the fit
    is worth on images it has not seen (a fitted row is optimal on the fitting images only)."""
    from . import fit as F
    from .coeffgen import save_coeff_matrix
    init = load_coeff_npz(init_path)
    teacher = load_coeff_npz(teacher) if isinstance(teacher, (str, os.PathLike)) else teacher
    n, n_hold = int(sample_count), int(sample_count if holdout is None else holdout)
    if n < 1 or n_hold < 0:
        raise ValueError("fit_coeff_matrix: sample_count >= 1 and holdout >= 0")
    checked = {k: fit_kw[k] for k in ("rows", "order", "ridge", "constraint", "batch_size", "t_tol") if k in fit_kw}
    F._check_fit_args(init, teacher, checked.get("rows"), checked.get("order"), checked.get("ridge", 0.0), checked.get("constraint", "marginal"),
                      checked.get("batch_size", 256), checked.get("t_tol", 1e-6))           # refusals before the first draw
    noise = philox_noise(range(n), (3, 32, 32), seed, device)
    C, B, node, report = F.fit_matrix(model_fn, init, teacher, noise, seed=seed, **fit_kw)
    report.update(C=C, B=B, node=node)
    if n_hold:
        held = philox_noise(range(n, n + n_hold), (3, 32, 32), seed, device)
        kw = {k: fit_kw[k] for k in ("batch_size", "t_tol") if k in fit_kw}
        m_fit, m_init = F.final_mse(model_fn, [(C, B, node), init], teacher, held, seed=seed, **kw)
        report["holdout"] = dict(n=n_hold, indices=(n, n + n_hold - 1), init_mse=m_init, fit_mse=m_fit, ratio=m_fit / m_init if m_init > 0 else float("nan"))
    if out_path is not None:
        save_coeff_matrix(out_path, C, B, node)
    return report


def save_neighbour_sheet(imgs, ref_imgs, idx, path, count: int = 16) -> None:
    """One PNG of the first ``count`` images (uint8 [n, H, W, 3]), one per line, each followed by its k neighbours ``ref_imgs[idx[i, t]]`` (nearest first;
    a slot without a neighbour, idx -1, stays black): ``count`` lines of 1 + k tiles with 2 pixels of black padding, (2 + count (H + 2)) x (2 + (1 + k) (W + 2))
    pixels."""
    from .ValidateNaturalInference import write_png_rgb
    to_np = lambda v: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)
    imgs, ref_imgs, idx = to_np(imgs), to_np(ref_imgs), to_np(idx)
    if idx.ndim != 2 or idx.shape[0] != imgs.shape[0] or imgs.ndim != 4 or imgs.shape[1:] != ref_imgs.shape[1:] or imgs.shape[3] != 3:
        raise ValueError("nearest: the sheet takes uint8 [n, H, W, 3] images, reference images of the same size and idx [n, k]")
    if idx.size and (idx.min() < -1 or idx.max() >= ref_imgs.shape[0]):
        raise ValueError("nearest: idx points outside the reference images")
    rows, k = max(0, min(int(count), imgs.shape[0])), idx.shape[1]
    h, w, pad = imgs.shape[1], imgs.shape[2], 2
    sheet = np.zeros((pad + rows * (h + pad), pad + (1 + k) * (w + pad), 3), np.uint8)
    for i in range(rows):
        tiles = [imgs[i]] + [ref_imgs[j] if j >= 0 else None for j in idx[i]]
        for t, tile in enumerate(tiles):
            if tile is not None:
                y, x = pad + i * (h + pad), pad + t * (w + pad)
                sheet[y:y + h, x:x + w] = tile
    write_png_rgb(sheet, path)


def calc_kid(imgs, ref_feats, device, model=None, estimator: str = "blocks", max_block_size: int = 1024) -> dict:
    """dict(kid, std, n_blocks, estimator) of the images (uint8 [n, H, W, 3]) against the real images' pool3 features ``ref_feats`` (array or ``.npy`` path):
    the Kernel Inception Distance with the cubic kernel on the features ``calc_fid`` is computed from (kid.py; include/natinf_kid.h) -- unbiased, so the
    number for a few thousand images, where FID is not.  ``"blocks"`` is TF-GAN's estimate with its standard error and depends on the order of the images;
    ``"full"`` is the MMD^2 of the whole sets.  A missing reference file raises ``kid: blocked``."""
    from . import kid as K
    from .prdc import FeatureSet
    real = _ref_features(ref_feats, device, "kid")
    model = model or fid_inception(device, tuple(imgs.shape[1:3]))
    return K.kid(FeatureSet(real, device=device), FeatureSet(get_features(imgs, model, device), device=device), estimator=estimator,
                 max_block_size=max_block_size, group=K.LOCAL)        # this process's images only, whatever process group exists


def calc_kid_sharded(imgs, ref_feats, device, group=None, model=None, estimator: str = "blocks", max_block_size: int = 1024) -> dict:
    """``calc_kid`` for a batch-sharded run: every rank scores ITS images, the features are all-gathered in rank order as ``calc_prdc_sharded`` does, and
    ``kid(..., group=group)`` splits the sweeps over the ranks; every rank returns the same dict.  The block estimate is that of the gathered order."""
    from . import kid as K
    from .prdc import FeatureSet
    real = _ref_features(ref_feats, device, "kid")
    model = model or fid_inception(device, tuple(imgs.shape[1:3]))
    feats = _gather_features(get_features(imgs, model, device), device, group)
    return K.kid(FeatureSet(real, device=device), FeatureSet(feats, device=device), estimator=estimator, max_block_size=max_block_size, group=group)


def fid_inception_head(device):
    """The classifier head (``fc.weight``, ``fc.bias``: 1,008 classes on pool3) of the checkpoint ``fid_inception`` loads, as an ``iscore.ClassifierHead``
    on ``device``.  The same file lookup, and without the file the same ``fid: blocked``."""
    from .inception import load_fid_inception_head
    from .iscore import ClassifierHead
    path = inception_weights_path()
    if not path.exists():
        raise FileNotFoundError(f"fid: blocked -- Inception weights {path} missing (pytorch_fid's {INCEPTION_WEIGHTS}; set NATINF_INCEPTION_WEIGHTS)")
    return ClassifierHead(*load_fid_inception_head(path), device=device)


def _score_head(head, device, bias: bool):
    head = head or fid_inception_head(device)
    return head if bias else head.without_bias()


def calc_is(imgs, device, model=None, head=None, splits: int = 1, bias: bool = True) -> dict:
    """dict(is, std, log_is, splits, n) of the images (uint8 [n, H, W, 3]): the Inception Score of the reference's evaluation (its ``inception_score``
    beside FID and KID), from the pool3 features ``calc_fid`` is computed from and the checkpoint's classifier head (iscore.py; include/natinf_is.h).
    It needs no reference set.  ``head``: an ``iscore.ClassifierHead`` (default: ``fid_inception_head``, which raises ``fid: blocked`` without the file).

    ``bias=True`` scores the graph's logits W a + b: TF-GAN's ``classifier_score_from_logits`` on the network's logits output, which the reference's
    evaluation calls.  ``bias=False`` scores the bias-free logits W a: the original implementation of Salimans et al. multiplies pool3 by the weights of
    ``softmax/logits/MatMul`` and never adds the bias, and torch-fidelity follows it (its ``logits_unbiased``).  ``splits=10`` is the protocol of
    Salimans et al.: the mean and the population standard deviation of the scores of ten contiguous parts."""
    from . import iscore as I
    head = _score_head(head, device, bias)
    model = model or fid_inception(device, tuple(imgs.shape[1:3]))
    return I.inception_score(I.FeatureSet(get_features(imgs, model, device), device=device), head, splits=splits, group=I.LOCAL)


def calc_is_sharded(imgs, device, group=None, model=None, head=None, splits: int = 1, bias: bool = True) -> dict:
    """``calc_is`` for a batch-sharded run: every rank scores ITS images and keeps its features; only the integer class sums and one fp64 per image cross
    ranks (``iscore.inception_score(..., group=group)``).  Every rank returns the same dict: that of one process on rank 0's images, then rank 1's, ..."""
    from . import iscore as I
    head = _score_head(head, device, bias)
    model = model or fid_inception(device, tuple(imgs.shape[1:3]))
    return I.inception_score(I.FeatureSet(get_features(imgs, model, device), device=device), head, splits=splits, group=group)


class FidBlocked:
    """What ``natural_inference_tx(compute_fid=True)`` returns when the FID assets (Inception weights, ``cifar10_mu_sigma.npz``) are absent:
    the images it generated and the reason -- distinguishable from both a FID value (float) and the ``compute_fid=False`` result (a tensor)."""

    def __init__(self, images: torch.Tensor, reason: str):
        self.images, self.reason = images, reason

    def __repr__(self):
        return f"FidBlocked({tuple(self.images.shape)}, {self.reason!r})"


@torch.no_grad()
def natural_inference_tx(batch_size: int = 500,
                         ckpt_filename: Optional[str] = None,
                         weight_path: Optional[str] = None,
                         sample_count: int = 50 * 1000, seed: int = 888, device: str = "cuda:0",
                         compute_fid: bool = True, flat_params: Optional[torch.Tensor] = None, streams: int = 3,
                         x0_fix: Optional[str] = None, x0_ratio: float = 0.995, x0_max: float = 1.0,
                         lowres=None, sr_scale: Optional[int] = None, sr_final: str = "step"):
    """Reference :242-317: generate ``sample_count`` CIFAR10 images with the NI matrix at ``weight_path``
    and score them.  ``flat_params`` lets a caller supply weights directly (engine order) instead of the
    score_sde checkpoint.

    ``streams`` (default 3 since round 6; 2 before): the batches are independent trajectories (reference loop :287-309); consecutive batches rotate over that many HIP streams
    (one engine handle + history buffer each), so that the under-occupied launches of one batch -- the 4x4 level, the per-sample GroupNorm
    tables, every launch's last round of blocks -- run under the other batch's convolutions: -6 % per batch at 512 images on one MI355X.
    The noise is drawn in the reference's order and every batch runs the same launches: the images are bit-identical to ``streams=1``,
    the reference's one-after-the-other order (tests/test_gpu_ncsnpp.py; DESIGN.md section 5 for what that took).

    ``x0_fix`` / ``x0_ratio`` / ``x0_max``: the x0 correction of ``generate_sharded`` ("clip" or "dynamic" thresholding of every step's predicted x0;
    DESIGN.md section 3i), refused on the host when a value is bad; ``None`` (default) is the reference's sampler.

    ``lowres`` / ``sr_scale`` / ``sr_final``: the super-resolution of ``generate_sharded``; a per-image ``lowres`` holds one row for each of the
    ``ceil(sample_count / batch_size) * batch_size`` images the loop generates.  Refused on the host when a value is bad; ``None`` (default) is the reference's sampler."""
    check_x0_fix(x0_fix, x0_ratio, x0_max, seed=seed, elems_per_image=3 * 32 * 32)
    if _check_sr_job(lowres, sr_scale, sr_final, seed=seed, x0_fix=x0_fix):
        lowres = prepare_lowres(lowres, sr_scale, int(np.ceil(sample_count / batch_size)) * batch_size)
    from .ncsnpp import NCSNppEngine, load_score_sde_checkpoint
    ckpt_filename = ckpt_filename or str(root_path / "deps/score_sde_pytorch/checkpoint_8.pth")
    weight_path = weight_path or str(root_path / "weights/step_5_weight_00.npz")
    if flat_params is None:
        assert os.path.exists(ckpt_filename)
        flat_params = load_score_sde_checkpoint(ckpt_filename)
    C, B, node = load_coeff_npz(weight_path)
    print(C / np.diag(C)[:, None])
    print(weight_path)
    bz = batch_size
    num = int(np.ceil(sample_count / bz))
    engine = NCSNppEngine(flat_params, max_batch=batch_size, device=device)
    lanes = BatchLanes(_lane_models(engine, streams, num), C, B, node, device, seed=seed, x0_fix=x0_fix, x0_ratio=x0_ratio, x0_max=x0_max,
                       sr_scale=sr_scale)                                             # the second lane shares the first's packed weights
    rows = KnownRows(torch.device(device), low=lowres) if sr_scale is not None else None
    torch.cuda.synchronize(torch.device(device))
    torch.manual_seed(seed)
    for ii in range(num):
        print("processing", ii)
        noise = torch.randn(bz, 3, 32, 32, dtype=torch.float32, device=device)      # the reference's stream of normals, in its order (:290)
        kw = dict(rows.batch(range(ii * bz, ii * bz + bz)), sr_final=sr_final) if rows is not None else {}
        lanes.submit(bz, noise=noise, index=ii * bz, **kw)                            # (stochastic matrices: image b of batch ii is ii*bz + b)
    all_batch = torch.concatenate(lanes.finish()).cpu()                                # ONE copy to the host, after the last batch
    if not compute_fid:
        return all_batch
    try:
        fid_value = calc_fid(all_batch, root_path / "weights/cifar10_mu_sigma.npz", device)
    except FileNotFoundError as e:                          # the assets are downloads: say so, keep the images
        print(e)
        return FidBlocked(all_batch, str(e))
    print(fid_value)
    print(weight_path)
    print(C / np.diag(C)[:, None])
    return fid_value


if __name__ == "__main__":
    natural_inference_tx()
