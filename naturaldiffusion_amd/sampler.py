"""Stateful Natural Inference samplers: one fused ``ni_step`` launch per sampling step.

Each class owns the history slab(s) in HBM ([slot][E], one coalesced stream per history row) and the
device-resident sparse coefficient rows, and mirrors one of the reference's three loop bodies:

* :class:`CifarNI`    -- src/CIFAR10NaturalInference.py:292-304 (fp64 history)
* :class:`ValidateNI` -- src/ValidateNaturalInference.py:349-366 (fp32 products, fp64 accumulate)
* :class:`SD3NI`      -- src/SD3NaturalInference.py:201-221 and :105-129 (fp16 chain)

Host code only sequences launches; all arithmetic is in libnatinf.so (include/natinf.h).
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ptr, stream_ptr
from .coeff import SparseRows, is_stochastic


def vp_std_f32(t: float, beta_0: float = 0.1, beta_1: float = 20.0) -> float:
    """sigma(t) of the VP SDE exactly as ``score_fn`` evaluates it (sde_lib.py:141-145 on the fp32
    vector ``t*ones``): host-side scalar schedule, fp32 torch ops on CPU."""
    vt = torch.ones(1, dtype=torch.float32) * t
    lmc = -0.25 * vt ** 2 * (beta_1 - beta_0) - 0.5 * vt * beta_0
    return float(torch.sqrt(1.0 - torch.exp(2.0 * lmc))[0])


def image_index_args(index, n_images: int, device):
    """The global image indices of a batch as the noise-generating steps take them -> (index tensor or None, first index,
    index stride).  ``index``: an int64 device tensor with one entry per image, an int ``first`` (image i is ``first + i``),
    a pair ``(first, stride)`` (image i is ``first + i*stride``) or None (= 0)."""
    if index is None:
        return None, 0, 1
    if isinstance(index, torch.Tensor):
        if (index.dtype != torch.int64 or index.device != device or not index.is_contiguous()
                or index.numel() != n_images):
            raise ValueError("index must be a contiguous int64 tensor on the sampler's device, one entry per image")
        return index, 0, 0
    if isinstance(index, (tuple, list)):
        return None, int(index[0]), int(index[1])
    return None, int(index), 1


def _pingpong(bufs, k: int, src: torch.Tensor) -> torch.Tensor:
    """The output buffer of step k: ``bufs[k & 1]``, or the other one when that is the step's input ``src``."""
    out = bufs[k & 1]
    return bufs[(k + 1) & 1] if out.data_ptr() == src.data_ptr() else out


def _check_elems_per_image(epi: Optional[int], E: int, lanes: int = 4) -> None:
    if epi is not None and (epi <= 0 or epi % lanes or E % epi):
        raise ValueError(f"elems_per_image must be a positive multiple of {lanes} dividing the element count")


def _level_memo(schedule: Callable) -> Callable:
    """``level(j, mode)`` = entry j of ``schedule(mode)``, each mode's list made on first use and kept (the samplers' known / colour levels)"""
    made = {}

    def level(j: int, mode: str):
        if mode not in made:
            made[mode] = schedule(mode)
        return made[mode][j]
    return level


def _check_guidance_tensors(cfg, uncond_slot, n: int, device) -> None:
    """per-image guidance as the guided and inpainting entries take it: fp32 scales and int32 slots, one of each per image, on the sampler's device"""
    if cfg.dtype != torch.float32 or cfg.device != device or not cfg.is_contiguous() or cfg.numel() != n:
        raise ValueError("a tensor cfg must be a contiguous fp32 tensor on the sampler's device, one scale per image")
    if (not isinstance(uncond_slot, torch.Tensor) or uncond_slot.dtype != torch.int32 or uncond_slot.device != device
            or not uncond_slot.is_contiguous() or uncond_slot.numel() != n):
        raise ValueError("a tensor cfg needs uncond_slot: a contiguous int32 tensor on the sampler's device, one slot per image")


def _flat_noise_f32(noise: torch.Tensor, n_elem: int) -> torch.Tensor:
    noise = noise.reshape(-1)
    if noise.dtype != torch.float32 or noise.numel() != n_elem or not noise.is_contiguous():
        raise ValueError("noise must be a contiguous fp32 tensor of n_elem elements")
    return noise


def _known_blend_f32(noise: torch.Tensor, known, mask, n_elem: int, epi, seed, level: Callable, known_final: str, index, fast_f32: bool = False):
    """``CifarNI.first_input`` / ``ValidateNI.first_input``: flat ``noise`` with the known elements at level 0 of ``level`` -> a new flat tensor"""
    ks, ms = check_known(known, mask, n_elem, epi, seed=seed, fast_f32=fast_f32, device=noise.device)
    ka, kstd, kcol = level(0, known_final)
    index, first, stride = image_index_args(index, n_elem // epi, noise.device)
    out = torch.empty_like(noise)
    check(lib.natinf_known_blend_f32(ptr(noise), ptr(out), ptr(known), ptr(mask), ks, ms, ka, kstd, kcol, seed,
                                     ptr(index), first, stride, epi, n_elem, stream_ptr()), "natinf_known_blend_f32")
    return out


KNOWN_COLUMN0 = 2 ** 31      # Philox column of the known-pixel draw at level 0; level j draws column KNOWN_COLUMN0 + j (a matrix's noise columns are <= N + 1)


def known_schedule(node: np.ndarray, known_final: str = "mean"):
    """The inpainting schedule of a node table [N+1, 3] (t, alpha, sigma) -> N + 1 triples (alpha fp32, std fp32, Philox column), as Python
    floats / ints.  Entry 0 is the level of the first model input; entry k + 1 is what step k blends with: the level of x_{k+1}, the node
    table's own.  The last entry draws nothing: ``known_final="mean"`` gives alpha_N * known (the reference returns
    ``x_mean``), ``"data"`` gives the known pixels back as they were given (alpha 1)."""
    if known_final not in ("mean", "data"):
        raise ValueError('known_final must be "mean" or "data"')
    node = np.asarray(node, np.float64)
    n = node.shape[0] - 1
    out = [(float(np.float32(node[j, 1])), float(np.float32(node[j, 2])), KNOWN_COLUMN0 + j) for j in range(n + 1)]
    out[n] = (out[n][0] if known_final == "mean" else 1.0, 0.0, KNOWN_COLUMN0 + n)
    return out


def _check_known(known, mask, n_elem: int, elems_per_image: Optional[int], dtype, lanes: int, own, epi_hint: str, device):
    """What ``check_known`` and ``check_known_f16`` share -> (known image stride, mask image stride).  ``own``: the caller's own refusals as
    (condition, message) pairs, raised where they always were: behind the both-or-neither check, in front of everything else."""
    if known is None or mask is None:
        raise ValueError("inpainting needs both known= and mask=")
    for bad, message in own:
        if bad:
            raise ValueError(message)
    if elems_per_image is None:
        raise ValueError(f"inpainting: {epi_hint}")
    epi = int(elems_per_image)
    _check_elems_per_image(epi, n_elem, lanes)
    strides = []
    for name, t, dt in (("known", known, dtype), ("mask", mask, torch.uint8)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{name} must be a flat contiguous {str(dt).split('.')[-1]} tensor")
        if t.numel() not in (n_elem, epi):
            raise ValueError(f"{name} must have n_elem ({n_elem}) or elems_per_image ({epi}) elements, not {t.numel()}")
        if device is not None and t.device != device:
            raise ValueError(f"{name} must be on the sampler's device")
        strides.append(epi if t.numel() == n_elem and n_elem != epi else 0)
    return strides[0], strides[1]


def check_known(known, mask, n_elem: int, elems_per_image: Optional[int], *, seed, fast_f32: bool = False, device=None):
    """The argument checks of an inpainting call, made before anything is launched -> (known image stride, mask image stride).
    ``known``: flat contiguous fp32, ``mask``: flat contiguous uint8 (non-zero = known), each of ``n_elem`` elements (one row per image:
    stride ``elems_per_image``) or ``elems_per_image`` elements (one row shared by every image: stride 0).  ``device`` None skips the
    device check (host-side callers)."""
    own = ((fast_f32, "inpainting: the fast_f32 mode has no blend"),
           (seed is None, "inpainting: the known pixels are re-noised at every level, which needs a seed (deterministic matrices too)"))
    return _check_known(known, mask, n_elem, elems_per_image, torch.float32, 4, own, "elems_per_image is needed to key the known-pixel noise", device)


def sd_known_schedule(sig16, oms16, renoise: str = "fresh"):
    """The inpainting schedule of the SD3 (flow) form -> N + 1 triples (sig, 1 - sig, Philox column) from the sampler's fp16-rounded sigma tables
    (``SD3NI.sig`` / ``SD3NI.oms``, N + 1 entries each).  Entry 0 is the level of the first model input; entry k + 1 is what step k blends with:
    the step's own ``sig_next`` / ``one_minus_sig_next``.  ``renoise="fresh"``: level j re-noises the known latents with a new draw, column
    ``KNOWN_COLUMN0 + j``; ``"same"``: with the image's own initial noise at every level, column 0."""
    if renoise not in ("fresh", "same"):
        raise ValueError('renoise must be "fresh" or "same"')
    if len(sig16) != len(oms16):
        raise ValueError("sig16 and oms16 must have the same length")
    return [(float(s), float(o), KNOWN_COLUMN0 + j if renoise == "fresh" else 0) for j, (s, o) in enumerate(zip(sig16, oms16))]


def check_known_f16(known, mask, n_elem: int, elems_per_image: Optional[int], *, seed, renoise: str = "fresh", device=None):
    """``check_known`` for the fp16 form (natinf_known_blend_f16 / natinf_step_f16chain_inpaint), made before anything is launched -> (known image
    stride, mask image stride).  ``known``: flat contiguous fp16, ``mask``: flat contiguous uint8 (non-zero = known) whose storage is 8-byte
    aligned, each of ``n_elem`` elements (one row per image) or ``elems_per_image`` elements (one row shared by every image: stride 0).  A seed is
    needed for ``renoise="fresh"`` only.  ``device`` None skips the device check (host-side callers)."""
    own = ((renoise not in ("fresh", "same"), 'renoise must be "fresh" or "same"'),
           (renoise == "fresh" and seed is None, 'inpainting: renoise="fresh" draws new noise for the known latents at every level, which needs a seed'))
    strides = _check_known(known, mask, n_elem, elems_per_image, torch.float16, 8, own,
                           "elems_per_image (sample_elems) is needed to key the known-latent noise", device)
    if mask.data_ptr() % 8:
        raise ValueError("mask must be 8-byte aligned: the step reads one 64-bit word per 8 elements")
    return strides


# Colorization.  COLOR_M: the orthonormal basis of deps/score_sde_pytorch/controllable_generation.py:107-109, fp32, whose column 0 is the
# gray direction: latent channel j of a pixel (R, G, B) is sum_i x_i * M[i][j].  COLOR_W = fp32(inv(fp64(COLOR_M))), as shortest round-trip literals
# (it differs from fp32 torch.inverse(M) in one entry by one ulp; max |M W - I| = 2.6e-8 in fp64).  The library takes both as arguments.
COLOR_M = np.array([[5.7735014e-01, -8.1649649e-01, 4.7008697e-08],
                    [5.7735026e-01, 4.0824834e-01, 7.0710671e-01],
                    [5.7735026e-01, 4.0824822e-01, -7.0710683e-01]], dtype=np.float32)
COLOR_W = np.array([[5.7735032e-01, 5.7735032e-01, 5.7735026e-01],
                    [-8.1649673e-01, 4.0824834e-01, 4.0824822e-01],
                    [6.8825528e-08, 7.0710677e-01, -7.0710683e-01]], dtype=np.float32)
COLOR_COLUMN0 = 2 ** 31 + 2 ** 30      # Philox column of the gray-channel draw at level 0; level j draws COLOR_COLUMN0 + j: disjoint from the matrix's columns and from KNOWN_COLUMN0 + j for N < 2^30


def color_schedule(node: np.ndarray, known_final: str = "mean"):
    """``known_schedule``'s levels with the colorization columns: N + 1 triples (alpha fp32, std fp32, COLOR_COLUMN0 + j); the last entry draws
    nothing ("mean": alpha_N * gray_u, "data": gray_u as given)."""
    return [(a, s, c - KNOWN_COLUMN0 + COLOR_COLUMN0) for a, s, c in known_schedule(node, known_final)]


def _dot3(a, b, c, p, q, r):
    """fp32(fp32(fp32(a*p) + fp32(b*q)) + fp32(c*r)) on fp32 numpy arrays and fp32 scalars: numpy rounds every operation to fp32"""
    return (a * p + b * q) + c * r


def decouple0_host(known) -> np.ndarray:
    """Latent channel 0 (the gray value) of centred fp32 pictures [..., 3, H, W] -> fp32 [..., H, W]: dot3(k0, k1, k2; M[0][0], M[1][0], M[2][0])."""
    k = np.asarray(known, dtype=np.float32)
    if k.ndim < 3 or k.shape[-3] != 3:
        raise ValueError("decouple0_host takes [..., 3, H, W]")
    M = COLOR_M
    return _dot3(k[..., 0, :, :], k[..., 1, :, :], k[..., 2, :, :], M[0, 0], M[1, 0], M[2, 0])


def color_blend_host(x, gray_u, alpha, std, z0=None, M=COLOR_M, W=COLOR_W) -> np.ndarray:
    """The colorization blend in numpy fp32, operation for operation the library's (include/natinf.h, natinf_color_blend_f32): ``x`` fp32 [..., 3, P],
    ``gray_u`` and ``z0`` (the normals of plane 0; not read when std == 0) fp32 broadcastable to [..., P] -> fp32 [..., 3, P].  The CPU replay of a
    GPU step, and what the GPU is compared against bit for bit."""
    x = np.asarray(x, dtype=np.float32)
    a, s = np.float32(alpha), np.float32(std)
    x0, x1, x2 = x[..., 0, :], x[..., 1, :], x[..., 2, :]
    u1 = _dot3(x0, x1, x2, M[0, 1], M[1, 1], M[2, 1])
    u2 = _dot3(x0, x1, x2, M[0, 2], M[1, 2], M[2, 2])
    u0 = np.asarray(gray_u, dtype=np.float32) * a
    if s != 0:
        u0 = u0 + np.asarray(z0, dtype=np.float32) * s
    out = np.stack([_dot3(u0, u1, u2, W[0, i], W[1, i], W[2, i]) for i in range(3)], axis=-2)
    assert out.dtype == np.float32
    return out


def _f9(m):
    """a 3x3 matrix as the ``const float[9]`` host array the colorization entries read at call time (row-major)"""
    import ctypes
    return (ctypes.c_float * 9)(*np.asarray(m, dtype=np.float32).reshape(-1).tolist())


def check_gray(gray_u, n_elem: int, elems_per_image: Optional[int], *, seed, fast_f32: bool = False, device=None) -> int:
    """The argument checks of a colorization call, made before anything is launched -> the gray image stride.  ``gray_u``: flat contiguous fp32,
    one value per pixel: ``n_elem / 3`` elements (one row per image: stride ``elems_per_image / 3``) or ``elems_per_image / 3`` (one picture shared by
    every image: stride 0).  ``device`` None skips the device check (host-side callers)."""
    if fast_f32:
        raise ValueError("colorization: the fast_f32 mode has no blend")
    if seed is None:
        raise ValueError("colorization: the gray channel is re-noised at every level, which needs a seed (deterministic matrices too)")
    if elems_per_image is None:
        raise ValueError("colorization: elems_per_image is needed to key the gray-channel noise")
    epi = int(elems_per_image)
    _check_elems_per_image(epi, n_elem)
    if epi % 12:
        raise ValueError("colorization: an image is three planes of whole quads (elems_per_image % 12 == 0)")
    if not isinstance(gray_u, torch.Tensor) or gray_u.dtype != torch.float32 or gray_u.dim() != 1 or not gray_u.is_contiguous():
        raise ValueError("gray_u must be a flat contiguous float32 tensor")
    if gray_u.numel() not in (n_elem // 3, epi // 3):
        raise ValueError(f"gray_u must have n_elem / 3 ({n_elem // 3}) or elems_per_image / 3 ({epi // 3}) elements, not {gray_u.numel()}")
    if device is not None and gray_u.device != device:
        raise ValueError("gray_u must be on the sampler's device")
    return epi // 3 if gray_u.numel() == n_elem // 3 and n_elem != epi else 0


# x0 correction: the modes of natinf_x0_threshold_f64 / natinf_step_f64hist_x0fix by the names the samplers take
X0_FIX_MODES = {"clip": _lib.X0_CLIP, "dynamic": _lib.X0_DYNAMIC}
X0_FIX_MAX_ELEMS = 8192      # one workgroup holds an image's fp64 x0 in LDS


def check_x0_fix(x0_fix, x0_ratio, x0_max, *, seed=0, elems_per_image: Optional[int] = 4, fast_f32: bool = False, gray: bool = False,
                 epi_later: bool = False) -> int:
    """The argument checks of an x0 correction, made before anything is launched -> the mode (0 for ``x0_fix=None``, which checks nothing
    else).  ``seed`` / ``elems_per_image``: pass the sampler's own (None is refused; ``epi_later``: a missing ``elems_per_image`` may still come
    with the step); host-side callers that have neither leave the defaults."""
    if x0_fix is None:
        return 0
    if not isinstance(x0_fix, str) or x0_fix not in X0_FIX_MODES:
        raise ValueError('x0_fix must be None, "clip" or "dynamic"')
    try:
        ratio, mx = float(x0_ratio), float(x0_max)
    except (TypeError, ValueError):
        raise ValueError("x0_ratio and x0_max must be numbers") from None
    if not 0.0 <= ratio <= 1.0:
        raise ValueError("x0_ratio must be in [0, 1]")
    if not (mx > 0.0 and math.isfinite(mx)):
        raise ValueError("x0_max must be positive and finite")
    if fast_f32:
        raise ValueError("x0_fix: the fast_f32 mode has no correction")
    if gray:
        raise ValueError("x0_fix does not go with gray_u (colorization): its step has one thread per pixel quad, the correction one workgroup per image")
    if seed is None:
        raise ValueError("x0_fix: the step takes the noise-drawing form, which needs a seed (deterministic matrices too)")
    if elems_per_image is None and not epi_later:
        raise ValueError("x0_fix: elems_per_image is needed, the threshold is a per-image statistic")
    if elems_per_image is not None and int(elems_per_image) > X0_FIX_MAX_ELEMS:
        raise ValueError(f"x0_fix: elems_per_image must be <= {X0_FIX_MAX_ELEMS}")
    return X0_FIX_MODES[x0_fix]


def _fma_f64(a: float, b: float, c: float) -> float:
    """fma(a, b, c) in fp64 with its one rounding: exact rational arithmetic for finite operands; a non-finite operand decides the result
    without any rounding, so the plain expression is right there"""
    from fractions import Fraction
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:                                                      # a zero product plus a zero is exact in plain arithmetic, sign included; a cancellation gives +0
        return float(np.float64(a) * np.float64(b) + np.float64(c)) if a == 0.0 or b == 0.0 else 0.0
    try:
        return float(exact)                                             # int / int true division: correctly rounded
    except OverflowError:
        return math.inf if exact > 0 else -math.inf


def x0_threshold_host(x0, mode, ratio: float = 0.995, max_val: float = 1.0):
    """The x0 correction in numpy fp64, operation for operation the library's (include/natinf.h, natinf_x0_threshold_f64): ``x0`` fp64
    [n_images, n] (or [n]: one image), ``mode`` "clip" / "dynamic" (or the ABI's 1 / 2) -> (y like ``x0``, s fp64 [n_images]).  The one fused
    multiply-add per image is evaluated exactly.  The CPU replay of a GPU step, and what the GPU is compared against byte for byte."""
    mode = X0_FIX_MODES.get(mode, mode)
    if mode not in (_lib.X0_CLIP, _lib.X0_DYNAMIC):
        raise ValueError('mode must be "clip" or "dynamic"')
    ratio, c = float(ratio), float(max_val)
    if not 0.0 <= ratio <= 1.0 or not (c > 0.0 and math.isfinite(c)):
        raise ValueError("ratio must be in [0, 1], max_val positive and finite")
    x = np.ascontiguousarray(x0, dtype=np.float64)
    rows = x.reshape(1, -1) if x.ndim == 1 else x.reshape(x.shape[0], -1)
    n = rows.shape[1]
    if mode == _lib.X0_CLIP:
        y = np.where(rows < -c, -c, np.where(rows > c, c, rows))        # a NaN fails both comparisons and stays, bits and all
        return y.reshape(x.shape), np.full(rows.shape[0], c)
    rank = ratio * float(n - 1)
    lo, hi = int(math.floor(rank)), int(math.ceil(rank))
    w = rank - lo
    y, s = np.empty_like(rows), np.empty(rows.shape[0])
    with np.errstate(invalid="ignore"):
        for i, r in enumerate(rows):
            a = np.sort(np.abs(r))                                       # NaN last
            a_lo, a_hi = float(a[lo]), float(a[hi])
            d = float(np.float64(a_hi) - np.float64(a_lo))
            q = _fma_f64(w, d, a_lo) if w < 0.5 else _fma_f64(w - 1.0, d, a_hi)
            s[i] = np.nan if np.isnan(r).any() or math.isnan(q) else max(q, c)
            y[i] = np.minimum(np.maximum(r, -s[i]), s[i]) / s[i]         # a NaN s makes every element NaN; inf / inf under an infinite s is one
    y[np.isnan(y)] = np.nan                                              # every NaN the correction produces: the one quiet pattern 0x7FF8000000000000
    return y.reshape(x.shape), s


# Super-resolution: the predicted x0 projected onto the pictures whose s x s block averages are the given low-resolution picture
SR_SCALES = (2, 4, 8)
SR_MAX_ELEMS = X0_FIX_MAX_ELEMS      # the same kernel shape: one workgroup holds an image's fp64 x0 in LDS
_QNAN = np.uint64(0x7FF8000000000000)
_INF_KEY = np.uint64(0x7FF0000000000000)


def _sr_geometry(shape, scale):
    """(C, H, W) and s of a projection, checked -> (C, H, W, s) as ints"""
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or int(scale) not in SR_SCALES:
        raise ValueError("sr_scale must be 2, 4 or 8")
    try:
        ok = len(shape) == 3 and all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) for v in shape)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("image_shape must be (channels, height, width)")
    c, h, w, s = int(shape[0]), int(shape[1]), int(shape[2]), int(scale)
    if c <= 0 or h <= 0 or w <= 0:
        raise ValueError("image_shape must be positive")
    if h % s or w % s:
        raise ValueError(f"image_shape: height and width must be multiples of sr_scale ({s})")
    if (c * h * w) % 4 or c * h * w > SR_MAX_ELEMS:
        raise ValueError(f"image_shape: channels*height*width must be a multiple of 4 and <= {SR_MAX_ELEMS}")
    return c, h, w, s


def downsample_host(x, shape, scale) -> np.ndarray:
    """The s x s block average A of NCHW images in numpy fp64, in the library's order (include/natinf.h, natinf_x0_project_f64): each block row added left
    to right, the row sums top to bottom, neither sum seeded with a zero, one multiplication by 2^(-2 log2 s).  ``x``: [..., C*H*W] (or [..., C, H, W]),
    ``shape`` = (C, H, W) -> fp64 [n, C*(H/s)*(W/s)], or 1-d for one flat image."""
    c, h, w, s = _sr_geometry(shape, scale)
    a = np.ascontiguousarray(x, dtype=np.float64)
    if a.size == 0 or a.size % (c * h * w):
        raise ValueError("downsample_host: x must hold whole images of image_shape")
    v = a.reshape(-1, c, h // s, s, w // s, s)
    with np.errstate(invalid="ignore", over="ignore"):
        rows = v[..., 0]
        for i in range(1, s):
            rows = rows + v[..., i]                                      # [n, C, H/s, s, W/s]
        total = rows[:, :, :, 0, :]
        for j in range(1, s):
            total = total + rows[:, :, :, j, :]
        m = total * (1.0 / (s * s))
    m = m.reshape(v.shape[0], -1)
    return m[0] if a.ndim == 1 else m


def x0_project_host(x0, low, shape, scale):
    """The x0 projection in numpy fp64, operation for operation the library's (include/natinf.h, natinf_x0_project_f64): ``x0`` fp64 [n_images, C*H*W] (or
    one flat image), ``low`` fp64 [n_images, C*(H/s)*(W/s)] or one row shared by every image -> (y like ``x0``, r fp64 [n_images], the largest |low - A x0|
    of each image).  The CPU replay of a GPU step, and what the GPU is compared against byte for byte."""
    c, h, w, s = _sr_geometry(shape, scale)
    x = np.ascontiguousarray(x0, dtype=np.float64)
    rows = x.reshape(-1, c * h * w)
    nblk = c * (h // s) * (w // s)
    lo = np.ascontiguousarray(low, dtype=np.float64).reshape(-1, nblk)
    if lo.shape[0] not in (1, rows.shape[0]):
        raise ValueError("x0_project_host: low must hold one row per image or one shared row")
    with np.errstate(invalid="ignore", over="ignore"):
        d = lo - downsample_host(rows, shape, scale)                     # [n, nblk]
        up = np.broadcast_to(d.reshape(-1, c, h // s, 1, w // s, 1), (rows.shape[0], c, h // s, s, w // s, s))
        y = rows.reshape(up.shape) + up
    y = np.ascontiguousarray(y).reshape(rows.shape)
    y[np.isnan(y)] = np.nan                                              # every NaN the projection produces: the one quiet pattern 0x7FF8000000000000
    keys = np.ascontiguousarray(np.abs(d)).view(np.uint64).max(axis=1)  # non-negative doubles order as their patterns, a NaN above +inf
    r = np.where(keys > _INF_KEY, _QNAN, keys).astype(np.uint64).view(np.float64)
    return y.reshape(x.shape), r


def check_project(sr_scale, image_shape, *, seed=0, elems_per_image: Optional[int] = None, fast_f32: bool = False, x0_fix=None,
                  conditioned: bool = False, epi_later: bool = False) -> int:
    """The argument checks of a super-resolution call, made before anything is launched -> the scale (0 for ``sr_scale=None``, which checks nothing
    else).  ``seed`` / ``elems_per_image``: pass the sampler's own (None is refused; ``epi_later``: a missing ``elems_per_image`` may still come with the
    step); ``conditioned``: known / mask / gray_u were given, which the projection does not go with; ``x0_fix``: the sampler's correction, likewise."""
    if sr_scale is None:
        return 0
    c, h, w, s = _sr_geometry(image_shape, sr_scale)
    if fast_f32:
        raise ValueError("sr_scale: the fast_f32 mode has no projection")
    if x0_fix is not None:
        raise ValueError("sr_scale does not go with x0_fix: the two act on the same predicted x0 and are not composed")
    if conditioned:
        raise ValueError("sr_scale does not go with known / mask (inpainting) or gray_u (colorization)")
    if seed is None:
        raise ValueError("sr_scale: the step takes the noise-drawing form, which needs a seed (deterministic matrices too)")
    if elems_per_image is None and not epi_later:
        raise ValueError("sr_scale: elems_per_image is needed, the projection is a per-image operation")
    if elems_per_image is not None and int(elems_per_image) != c * h * w:
        raise ValueError(f"sr_scale: elems_per_image ({int(elems_per_image)}) must be channels*height*width of image_shape ({c * h * w})")
    return s


def check_low(low, n_elem: int, elems_per_image: int, scale: int, device=None) -> int:
    """The low-resolution picture of a super-resolution step -> its image stride: flat contiguous fp64 of ``n_elem / s^2`` elements (one picture per image:
    stride ``elems_per_image / s^2``) or ``elems_per_image / s^2`` (one picture shared by every image: stride 0)."""
    per = int(elems_per_image) // (scale * scale)
    if not isinstance(low, torch.Tensor) or low.dtype != torch.float64 or low.dim() != 1 or not low.is_contiguous():
        raise ValueError("low must be a flat contiguous float64 tensor")
    if low.numel() not in (n_elem // (scale * scale), per):
        raise ValueError(f"low must have n_elem / s^2 ({n_elem // (scale * scale)}) or elems_per_image / s^2 ({per}) elements, not {low.numel()}")
    if device is not None and low.device != device:
        raise ValueError("low must be on the sampler's device")
    return per if low.numel() == n_elem // (scale * scale) and n_elem != elems_per_image else 0


class CifarNI:
    """x_{k+1} = fp32(sum_j C[k,j]*x0_j) + fp32(B[k,0])*noise with x0_k = ((-out/std)*sigma^2 + x_k)/alpha.

    A stochastic matrix (``coeff.is_stochastic``: some B[k, j >= 1] != 0) adds the noise injected after each step,
    fp32(sum_j fp32(B[k,j]*eps_j)) in fp64 accumulation, eps_0 = ``noise`` and eps_j (j >= 1) drawn in the kernel from
    Philox(``seed``, global image index, column j) (include/natinf.h, natinf_step_f64hist_noise).  It needs ``seed``;
    ``elems_per_image`` defaults to the per-image size of the noise ``run`` gets; the fp32 fast mode does not take it.

    Inpainting (``known=`` / ``mask=`` of ``step`` and ``run``; natinf_step_f64hist_inpaint): after every update the known pixels are
    overwritten, inside the step's launch, with the data diffused to the level of the step's output (``known_schedule``).  It needs a
    ``seed`` and ``elems_per_image`` for any matrix; a deterministic one goes through as a one-term noise row.

    Colorization (``gray_u=`` of ``first_input``, ``step`` and ``run``; natinf_step_f64hist_colorize): the same, on one channel of a rotated colour
    space instead of a subset of the pixels -- after every update latent channel 0 of every pixel (``COLOR_M``) is overwritten with ``gray_u``
    diffused to the level of the step's output (``color_schedule``).  ``gray_u`` together with ``known`` or ``mask`` is a ValueError.

    x0 correction (``x0_fix="clip"`` / ``"dynamic"``; natinf_step_f64hist_x0fix): every step corrects its predicted x0 per image before it enters
    the history and the sum -- clamped to [-``x0_max``, ``x0_max``] (DDPM's clip_denoised), or clamped to and divided by s = max(the ``x0_ratio``
    quantile of the image's |x0|, ``x0_max``) (Imagen's dynamic thresholding, the reference's ``correcting_x0_fn="dynamic_thresholding"``).  Matrix
    X with it is the classical solver X with that ``correcting_x0_fn``.  It needs a ``seed`` and ``elems_per_image`` (<= 8192) like inpainting,
    goes with ``known`` / ``mask``, and not with ``fast_f32`` or ``gray_u``.  ``x0_s`` [n_step, n_images] fp64 (device) holds the thresholds used
    (``"clip"``: ``x0_max``), row k written by step k.  ``x0_fix=None`` (default) launches exactly what the class launched without the option.

    Super-resolution (``sr_scale=2 | 4 | 8`` with ``image_shape=(C, H, W)``, and ``low=`` of ``step`` and ``run``; natinf_step_f64hist_project): every step
    projects its predicted x0 onto the pictures whose s x s block averages are ``low``, x0 <- x0 + up(low - A x0), before it enters the history and the
    sum.  Matrix X with it is the classical solver X run as DDNM (Wang et al. 2022), and every history row has the block means of the data.  It needs a
    ``seed`` and ``elems_per_image`` (= C*H*W <= 8192), and goes with none of ``fast_f32``, ``x0_fix``, ``known`` / ``mask`` and ``gray_u``.  ``sr_r``
    [n_step, n_images] fp64 (device) holds the largest |low - A x0| of each image, row k written by step k: how far each step's prediction was from the
    data.  ``sr_scale=None`` (default) launches exactly what the class launched without the option."""

    def __init__(self, C: np.ndarray, B: np.ndarray, node: np.ndarray, n_elem: int, device="cuda:0",
                 dense: bool = False, fast_f32: bool = False, stds=None, *, seed: Optional[int] = None,
                 elems_per_image: Optional[int] = None, x0_fix: Optional[str] = None, x0_ratio: float = 0.995, x0_max: float = 1.0,
                 sr_scale: Optional[int] = None, image_shape=None):
        # (the correction's and the projection's refusals come first: they need no GPU; elems_per_image may still come with the step)
        self.x0_mode = check_x0_fix(x0_fix, x0_ratio, x0_max, seed=seed, elems_per_image=elems_per_image, fast_f32=fast_f32, epi_later=True)
        self.sr_scale = check_project(sr_scale, image_shape, seed=seed, elems_per_image=elems_per_image, fast_f32=fast_f32, x0_fix=x0_fix, epi_later=True)
        self.image_shape, self.sr_r = (tuple(int(v) for v in image_shape) if self.sr_scale else None), None
        self.x0_fix, self.x0_ratio, self.x0_max, self.x0_s = x0_fix, float(x0_ratio), float(x0_max), None
        _lib.require_gpu()
        if n_elem % 4:
            raise ValueError("element count must be a multiple of 4")
        self.C, self.B, self.node = (np.asarray(a, np.float64) for a in (C, B, node))
        self.n_step = self.node.shape[0] - 1
        if self.C.shape != (self.n_step, self.n_step):
            raise ValueError("C must be [N,N] with N = len(node_coeff)-1")
        self.E = int(n_elem)
        self.device = torch.device(device)
        self.fast = bool(fast_f32)
        self.stochastic = is_stochastic(self.B)
        if self.stochastic:
            if seed is None:
                raise ValueError("stochastic NI matrix (B[k, j >= 1] != 0): the injected noise needs a seed")
            if self.fast:
                raise ValueError("stochastic NI matrix: fast_f32 mode only covers column 0 of B")
            _check_elems_per_image(elems_per_image, self.E)
            self.rows_b = SparseRows(self.B, lambda k: min(k + 2, self.B.shape[1]), torch.float32, self.device,
                                     diag=False, dense=dense)
        self.seed = None if seed is None else int(seed) & (2 ** 64 - 1)
        self.epi = None if elems_per_image is None else int(elems_per_image)
        hdt = torch.float32 if self.fast else torch.float64
        self.rows = SparseRows(self.C, lambda k: k + 1, hdt, self.device, dense=dense)
        self.hist = torch.empty((self.n_step, self.E), dtype=hdt, device=self.device)
        self._x = [torch.empty(self.E, dtype=torch.float32, device=self.device) for _ in range(2)]
        # fp32 VP std per step, evaluated on the host like score_fn does; `stds` lets a caller pin them
        # (torch.exp on CPU differs in the last ulp between hosts -- so does the reference's own value)
        self.std = [vp_std_f32(self.node[k, 0]) for k in range(self.n_step)] if stds is None else [float(v) for v in stds]
        self.labels = [float(np.float32(self.node[k, 0]) * np.float32(999)) for k in range(self.n_step)]
        self._rows_b0 = None
        self._known_level = _level_memo(lambda known_final: known_schedule(self.node, known_final))
        self._color_level = _level_memo(lambda known_final: color_schedule(self.node, known_final))

    def _noise_rows(self) -> SparseRows:
        """The noise rows an inpainting step passes: B's own for a stochastic matrix, else column 0 alone as a one-term row
        (val_b[0] = fp32(B[k,0]): natinf_step_f64hist's bytes), made on first use."""
        if self.stochastic:
            return self.rows_b
        if self._rows_b0 is None:
            self._rows_b0 = SparseRows(self.B[:, :1], lambda k: 1, torch.float32, self.device, diag=False, dense=True)
        return self._rows_b0

    def first_input(self, noise: torch.Tensor, known: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, index=None,
                    elems_per_image: Optional[int] = None, known_final: str = "mean", *, gray_u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The first model input of an inpainting trajectory: ``noise`` with the known pixels at level 0 (natinf_known_blend_f32,
        column 2^31) -> a new flat tensor; ``noise`` itself (eps_0 of every step) is left as it is.  With ``gray_u`` (colorization) it is
        ``noise`` with its gray channel at level 0 (natinf_color_blend_f32, column ``COLOR_COLUMN0``)."""
        epi = self.epi if elems_per_image is None else int(elems_per_image)
        noise = _flat_noise_f32(noise, self.E)
        if gray_u is not None:
            if known is not None or mask is not None:
                raise ValueError("gray_u (colorization) does not go with known / mask (inpainting)")
            gs = check_gray(gray_u, self.E, epi, seed=self.seed, fast_f32=self.fast, device=noise.device)
            ga, gstd, gcol = self._color_level(0, known_final)
            index, first, stride = image_index_args(index, self.E // epi, noise.device)
            out = torch.empty_like(noise)
            check(lib.natinf_color_blend_f32(ptr(noise), ptr(out), ptr(gray_u), gs, _f9(COLOR_M), _f9(COLOR_W), ga, gstd, gcol, self.seed,
                                             ptr(index), first, stride, epi, self.E, stream_ptr()), "natinf_color_blend_f32")
            return out
        return _known_blend_f32(noise, known, mask, self.E, epi, self.seed, self._known_level, known_final, index, fast_f32=self.fast)

    def step(self, k: int, x_k: torch.Tensor, model_out: torch.Tensor, noise: torch.Tensor,
             x_next: Optional[torch.Tensor] = None, index=None, elems_per_image: Optional[int] = None, *,
             known: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, known_final: str = "mean",
             gray_u: Optional[torch.Tensor] = None, low: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``index`` (stochastic matrices): the batch's global image indices -- an int64 device tensor with one entry per
        image, an int ``first`` (image i is ``first + i``) or a pair ``(first, stride)`` (image i is ``first + i*stride``);
        None = 0.  ``elems_per_image`` overrides the constructor's value for this call.

        ``known`` / ``mask`` (inpainting): flat fp32 / uint8 device tensors of ``n_elem`` elements (one row per image) or
        ``elems_per_image`` elements (one row for every image); a non-zero mask byte marks a known element, which leaves the step as
        ``known`` diffused to the level of x_{k+1} (``known_schedule``; ``known_final`` says what the last step leaves).  ``index`` keys
        that noise too.

        ``gray_u`` (colorization): a flat fp32 device tensor of ``n_elem / 3`` elements (one row per image) or ``elems_per_image / 3`` (one
        picture for every image): latent channel 0 of the known picture (``decouple0_host``), which leaves the step, in every pixel's latent
        channel 0, diffused to the level of x_{k+1} (``color_schedule``).  Not together with ``known`` / ``mask``.

        ``low`` (super-resolution, a sampler made with ``sr_scale``): a flat fp64 device tensor of ``n_elem / s^2`` elements (one low-resolution picture
        per image, [C][H/s][W/s]) or ``elems_per_image / s^2`` (one picture for every image).  Not together with ``known`` / ``mask`` / ``gray_u``."""
        epi = self.epi if elems_per_image is None else int(elems_per_image)
        inpaint = known is not None or mask is not None
        if self.sr_scale:                                                 # refusals first: conditioning, a missing or wrong elems_per_image, a bad low
            check_project(self.sr_scale, self.image_shape, seed=self.seed, elems_per_image=epi, conditioned=inpaint or gray_u is not None)
            _check_elems_per_image(epi, self.E)
            if low is None:
                raise ValueError("a sampler made with sr_scale needs low= at every step")
            ls = check_low(low, self.E, epi, self.sr_scale, device=x_k.device)
        elif low is not None:
            raise ValueError("low= belongs to a sampler made with sr_scale")
        if self.x0_mode:                                                  # refusals first: gray_u, a missing or oversized elems_per_image
            check_x0_fix(self.x0_fix, self.x0_ratio, self.x0_max, seed=self.seed, elems_per_image=epi, gray=gray_u is not None)
            _check_elems_per_image(epi, self.E)
        if gray_u is not None:                                            # refusals first, as for inpainting
            if inpaint:
                raise ValueError("gray_u (colorization) does not go with known / mask (inpainting)")
            gs = check_gray(gray_u, self.E, epi, seed=self.seed, fast_f32=self.fast, device=x_k.device)
            ga, gstd, gcol = self._color_level(k + 1, known_final)
        if inpaint:                                                       # refusals first: nothing below touches the GPU before them
            ks, ms = check_known(known, mask, self.E, epi, seed=self.seed, fast_f32=self.fast, device=x_k.device)
            ka, kstd, kcol = self._known_level(k + 1, known_final)
        if x_next is None:
            x_next = _pingpong(self._x, k, x_k)
        for t in (x_k, model_out, noise):
            if t.dtype != torch.float32 or t.numel() != self.E or not t.is_contiguous():
                raise ValueError("x_k / model_out / noise must be contiguous fp32 tensors of n_elem elements")
        idx, val, n = self.rows.ptrs(k)
        r = self.rows.rows[k]
        a, s = float(self.node[k, 1]), float(self.node[k, 2])
        if inpaint or gray_u is not None or self.stochastic or self.x0_mode or self.sr_scale:    # the entries that draw noise: B's rows and the images' global indices
            if epi is None:
                raise ValueError("stochastic NI matrix: elems_per_image is needed to key the injected noise")
            ib, vb, nb = self._noise_rows().ptrs(k)
            index, first, stride = image_index_args(index, self.E // epi, x_k.device)
            head = (ptr(x_k), ptr(model_out), ptr(noise), ptr(self.hist), ptr(x_next), idx, val, n, r.diag, ib, vb, nb, k, a, s, self.std[k],
                    self.seed, ptr(index), first, stride, epi, self.E)             # what the five natinf_step_f64hist_* noise entries share
        if self.sr_scale:
            n_images = self.E // epi
            if self.sr_r is None or self.sr_r.shape[1] != n_images:
                self.sr_r = torch.zeros((self.n_step, n_images), dtype=torch.float64, device=self.device)
            c, h, w = self.image_shape
            check(lib.natinf_step_f64hist_project(*head, ptr(low), ls, c, h, w, self.sr_scale, ptr(self.sr_r[k]), stream_ptr()),
                  "natinf_step_f64hist_project")
            return x_next
        if self.x0_mode:                                                  # with or without known pixels: one entry
            n_images = self.E // epi
            if self.x0_s is None or self.x0_s.shape[1] != n_images:
                self.x0_s = torch.zeros((self.n_step, n_images), dtype=torch.float64, device=self.device)
            kargs = (ptr(known), ptr(mask), ks, ms, ka, kstd, kcol) if inpaint else (0, 0, 0, 0, 0.0, 0.0, 0)
            check(lib.natinf_step_f64hist_x0fix(*head, *kargs, self.x0_mode, self.x0_ratio, self.x0_max, ptr(self.x0_s[k]), stream_ptr()),
                  "natinf_step_f64hist_x0fix")
            return x_next
        if inpaint:
            check(lib.natinf_step_f64hist_inpaint(*head, ptr(known), ptr(mask), ks, ms, ka, kstd, kcol, stream_ptr()),
                  "natinf_step_f64hist_inpaint")
            return x_next
        if gray_u is not None:
            check(lib.natinf_step_f64hist_colorize(*head, ptr(gray_u), gs, _f9(COLOR_M), _f9(COLOR_W), ga, gstd, gcol, stream_ptr()),
                  "natinf_step_f64hist_colorize")
            return x_next
        if self.stochastic:
            check(lib.natinf_step_f64hist_noise(*head, stream_ptr()), "natinf_step_f64hist_noise")
            return x_next
        b0 = float(np.float32(self.B[k, 0]))
        fn = lib.natinf_step_f32hist if self.fast else lib.natinf_step_f64hist
        check(fn(ptr(x_k), ptr(model_out), ptr(noise), ptr(self.hist), ptr(x_next), idx, val, n, r.diag, k,
                 a, s, self.std[k], b0, self.E, stream_ptr()), "natinf_step_f64hist")
        return x_next

    def run(self, model_fn: Callable, noise: torch.Tensor, return_all: bool = False, index=None, *,
            known: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, known_final: str = "mean",
            gray_u: Optional[torch.Tensor] = None, low: Optional[torch.Tensor] = None, sr_final: str = "step"):
        """``model_fn(x [B,...] fp32, labels [B] fp32) -> out`` (raw network output).  ``index``: see ``step``.
        ``known`` / ``mask`` (inpainting; any shape holding B or 1 images, ``mask`` uint8 or bool): the first model input is ``noise``
        with the known pixels at level 0, and every step blends (``step``); with ``return_all`` entry 0 is that first input.
        ``gray_u`` (colorization; any shape holding B or 1 gray pictures of one value per pixel): the same with the gray-channel blend.
        ``low`` (super-resolution; fp64, any shape holding B or 1 low-resolution pictures): every step projects its x0 (``step``).  ``sr_final="step"``
        returns x_N as every other job does; ``"x0"`` returns fp32(hist[N-1]), the last projected prediction -- what DDNM returns, and the only result
        whose block means are the data whatever the matrix's end level (with ``return_all`` it is appended behind x_N)."""
        shape, B = noise.shape, noise.shape[0]
        noise = noise.contiguous()
        epi = self.epi if self.epi is not None else noise.numel() // B
        inpaint = known is not None or mask is not None
        if sr_final not in ("step", "x0"):
            raise ValueError('sr_final must be "step" or "x0"')
        if self.sr_scale:
            check_project(self.sr_scale, self.image_shape, seed=self.seed, elems_per_image=epi, conditioned=inpaint or gray_u is not None)
            if low is None:
                raise ValueError("a sampler made with sr_scale needs low=")
        elif low is not None or sr_final != "step":
            raise ValueError('low= and sr_final="x0" belong to a sampler made with sr_scale')
        if gray_u is not None and inpaint:
            raise ValueError("gray_u (colorization) does not go with known / mask (inpainting)")
        if self.x0_mode:
            check_x0_fix(self.x0_fix, self.x0_ratio, self.x0_max, seed=self.seed, elems_per_image=epi, gray=gray_u is not None)
        # every step goes through self.step (callers wrap it per instance, e.g. bench.py's timed replica): a column-0 matrix gets exactly the four
        # positional arguments it always got, a stochastic one index= and elems_per_image=, a conditioned trajectory its blend arguments as well
        kw = dict(index=index, elems_per_image=epi) if self.stochastic or inpaint or gray_u is not None or self.x0_mode or self.sr_scale else {}
        if self.sr_scale:
            kw.update(low=low.reshape(-1))
        if gray_u is not None:
            kw.update(gray_u=gray_u.reshape(-1), known_final=known_final)
        elif inpaint:
            flat = lambda t: t if t is None else (t.view(torch.uint8) if t.dtype == torch.bool else t).reshape(-1)
            kw.update(known=flat(known), mask=flat(mask), known_final=known_final)
        x = self.first_input(noise, **kw) if inpaint or gray_u is not None else noise
        xs = [x.view(shape)]
        for k in range(self.n_step):
            labels = torch.full((B,), self.labels[k], dtype=torch.float32, device=self.device)
            out = model_fn(x.view(shape), labels)
            x = self.step(k, x.reshape(-1), out.contiguous().reshape(-1), noise.reshape(-1), **kw)
            if return_all:
                x = x.clone()
                xs.append(x.view(shape))
        if sr_final == "x0":
            x = self.hist[self.n_step - 1].to(torch.float32)
            xs.append(x.view(shape))
        return xs if return_all else x.view(shape)


class ValidateNI:
    """DiT / eps-prediction form with per-step fresh noise and CFG (ValidateNaturalInference.py:311-372).

    Without ``seed`` the caller fills the noise-history slab ``hist_eps`` (row 0 the initial noise, row j the draw after step
    j-1) and ``step`` is natinf_step_f32prod.  With ``seed`` there is no slab: ``step`` takes the initial noise and the batch's
    global image indices and draws eps_j, j >= 1, in the kernel from Philox(``seed``, global image index, column j)
    (include/natinf.h, natinf_step_f32prod_noise) -- the bytes of the slab path on a slab filled by ``philox_noise(column=j)``,
    for stochastic (``ddpm_*``) and deterministic (``ddim_*``: column 0 only) matrices alike.  ``elems_per_image`` pins the
    per-image size ``step`` must be called with (None: whatever ``sample_elems`` each call gives).  The seeded ``step`` also takes
    per-image guidance (``cfg`` a tensor with ``uncond_slot``: natinf_step_f32prod_noise_guided).

    Latent-space inpainting (``known=`` / ``mask=`` of the seeded ``step``, and ``first_input``; natinf_step_f32prod_inpaint): after every update
    the known latent elements are overwritten, inside the step's launch, with the known latents diffused to the level of the step's output
    (``known_schedule`` of the node table, whose rows are the marginal (alpha, sigma) of each level).  The slab form has no blend."""

    def __init__(self, C: np.ndarray, B: np.ndarray, node: np.ndarray, c1: np.ndarray, c2: np.ndarray, n_elem: int,
                 device="cuda:0", dense: bool = False, *, seed: Optional[int] = None, elems_per_image: Optional[int] = None):
        _lib.require_gpu()
        if n_elem % 4:
            raise ValueError("element count must be a multiple of 4")
        self.n_step = int(np.asarray(B).shape[0])
        self.node = np.asarray(node, np.float64)
        self.E = int(n_elem)
        self.device = torch.device(device)
        self.seed = None if seed is None else int(seed) & (2 ** 64 - 1)
        if elems_per_image is not None:
            if seed is None:
                raise ValueError("elems_per_image belongs to the seeded (in-kernel noise) form: give a seed")
            _check_elems_per_image(elems_per_image, self.E)
        self.epi = None if elems_per_image is None else int(elems_per_image)
        self.rows_c = SparseRows(C, lambda k: k + 1, torch.float32, self.device, dense=dense)
        self.rows_b = SparseRows(B, lambda k: min(k + 2, np.asarray(B).shape[1]), torch.float32, self.device, dense=dense, diag=False)
        self.c1 = [float(np.float32(v)) for v in c1]
        self.c2 = [float(np.float32(v)) for v in c2]
        self.hist_x0 = torch.empty((self.n_step, self.E), dtype=torch.float32, device=self.device)
        # the seeded form draws the noise rows in the kernel: no (N+1) x E slab
        self.hist_eps = None if self.seed is not None else torch.empty((self.n_step + 1, self.E), dtype=torch.float32, device=self.device)
        self._z = [torch.empty(self.E, dtype=torch.float32, device=self.device) for _ in range(2)]
        self._known_level = _level_memo(lambda known_final: known_schedule(self.node, known_final))
        self._launch_wide = {}

    def _launch_wide_guidance(self, n: int, cfg: float, have_uncond: bool):
        """A launch-wide scale in the per-image form the inpainting entry takes -> (scales fp32 [n], slots int32 [n]), built once per sampler:
        slots 0..n-1 with every scale ``cfg``, or every slot -1 without an unconditional half.  The guided entry's identity rule makes these the
        launch-wide form's bytes."""
        key = (n, float(cfg), bool(have_uncond))
        if key not in self._launch_wide:
            slots = torch.arange(n, dtype=torch.int32) if have_uncond else torch.full((n,), -1, dtype=torch.int32)
            self._launch_wide[key] = (torch.full((n,), float(cfg), dtype=torch.float32).to(self.device), slots.to(self.device))
        return self._launch_wide[key]

    def first_input(self, noise: torch.Tensor, known: torch.Tensor, mask: torch.Tensor, index=None, known_final: str = "mean",
                    elems_per_image: Optional[int] = None) -> torch.Tensor:
        """The first model input of an inpainting trajectory: ``noise`` with the known latents at level 0 (natinf_known_blend_f32, column
        ``KNOWN_COLUMN0``) -> a new flat tensor; ``noise`` itself (eps_0 of every step) is left as it is."""
        epi = self.epi if elems_per_image is None else int(elems_per_image)
        return _known_blend_f32(_flat_noise_f32(noise, self.E), known, mask, self.E, epi, self.seed, self._known_level, known_final, index)

    def step(self, k: int, z: torch.Tensor, cond: torch.Tensor, uncond: Optional[torch.Tensor], cfg,
             sample_elems: Optional[int] = None, eps_sample_stride: Optional[int] = None, *,
             noise: Optional[torch.Tensor] = None, index=None, uncond_slot: Optional[torch.Tensor] = None,
             n_uncond: Optional[int] = None, known: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
             known_final: str = "mean") -> torch.Tensor:
        """``noise`` / ``index`` (seeded form only): the initial noise eps_0 ([E] fp32, contiguous) and the batch's global image
        indices in one of ``image_index_args``' forms; an image is one sample of ``sample_elems`` elements.

        ``cfg`` a float: one scale for the launch, ``uncond`` row i belongs to image i (None: eps = cond).  ``cfg`` a tensor (seeded
        form only; natinf_step_f32prod_noise_guided): the per-image scales, fp32 ``[n]`` on the device, with ``uncond_slot`` int32 ``[n]``
        on the device -- image i's row in ``uncond``, or -1 for an unguided image (eps = cond, its scale is not read).  ``uncond`` then
        holds ``n_uncond`` samples at ``eps_sample_stride`` (default: ``uncond.numel() // eps_sample_stride``; None = no row).  The entry
        reads ``uncond_slot`` back before it launches: fill it before the call, once per batch.

        ``known`` / ``mask`` (seeded form only; natinf_step_f32prod_inpaint): flat fp32 / uint8 device tensors of ``n_elem`` elements (one row per
        image) or ``sample_elems`` elements (one row for every image); a non-zero mask byte marks a known latent element (one byte per ELEMENT:
        a per-cell mask is repeated over the channels by the caller), which leaves the step as ``known`` diffused to the level of z_{k+1}:
        level k + 1 of ``known_schedule(node, known_final)``, column ``KNOWN_COLUMN0 + k + 1``; the last level draws nothing.  ``index`` keys that
        noise too.  A float ``cfg`` goes through the per-image entry as slots 0..n-1 (all -1 for ``uncond=None``) with that scale: the same bytes."""
        se = self.E if sample_elems is None else int(sample_elems)
        st = se if eps_sample_stride is None else int(eps_sample_stride)
        guided = isinstance(cfg, torch.Tensor)
        inpaint = known is not None or mask is not None
        if inpaint:                                                       # refusals first: nothing below touches the GPU before them
            if self.seed is None:
                raise ValueError("known / mask belong to the seeded form: the slab form has no blend")
            ks, ms = check_known(known, mask, self.E, se, seed=self.seed, device=z.device)
            ka, kstd, kcol = self._known_level(k + 1, known_final)
        if guided and (self.seed is None or noise is None):
            raise ValueError("a tensor cfg (per-image scales) belongs to the seeded form with noise= / index=: the slab form takes one float")
        if not guided and (uncond_slot is not None or n_uncond is not None):
            raise ValueError("uncond_slot / n_uncond go with a tensor cfg (per-image scales)")
        z_next = _pingpong(self._z, k, z)
        ic, vc, nc = self.rows_c.ptrs(k)
        ib, vb, nb = self.rows_b.ptrs(k)
        if self.seed is None:
            if noise is not None or index is not None:
                raise ValueError("noise / index belong to the seeded form; without a seed the noises are read from hist_eps")
            check(lib.natinf_step_f32prod(ptr(z), ptr(cond), ptr(uncond), float(cfg), se, st, ptr(self.hist_x0),
                                          ptr(self.hist_eps), ptr(z_next), ic, vc, nc, self.rows_c.rows[k].diag,
                                          ib, vb, nb, k, self.c1[k], self.c2[k], self.E, stream_ptr()), "natinf_step_f32prod")
            return z_next
        if noise is None:
            raise ValueError("seeded form: step needs the initial noise (noise=); there is no hist_eps slab to read it from")
        if noise.dtype != torch.float32 or noise.numel() != self.E or not noise.is_contiguous() or noise.device != z.device:
            raise ValueError("noise must be a contiguous fp32 tensor of n_elem elements on the sampler's device")
        if se <= 0 or se % 4 or self.E % se or (self.epi is not None and se != self.epi):
            raise ValueError("sample_elems must be the per-image element count: a multiple of 4 dividing the element count"
                             + ("" if self.epi is None else f" (elems_per_image = {self.epi})"))
        index, first, stride = image_index_args(index, self.E // se, z.device)
        # what the three seeded natinf_step_f32prod_* entries share behind their guidance arguments
        tail = (se, st, ptr(self.hist_x0), ptr(noise), ptr(z_next), ic, vc, nc, self.rows_c.rows[k].diag, ib, vb, nb, k, self.c1[k], self.c2[k],
                self.seed, ptr(index), first, stride, self.E)
        if inpaint and not guided:
            cfg, uncond_slot = self._launch_wide_guidance(self.E // se, float(cfg), uncond is not None)
            n_uncond = self.E // se if uncond is not None else 0
        if guided or inpaint:
            _check_guidance_tensors(cfg, uncond_slot, self.E // se, z.device)
            if n_uncond is None:
                n_uncond = 0 if uncond is None else uncond.numel() // st
            if inpaint:
                check(lib.natinf_step_f32prod_inpaint(ptr(z), ptr(cond), ptr(uncond), ptr(cfg), ptr(uncond_slot), int(n_uncond), *tail,
                                                      ptr(known), ptr(mask), ks, ms, ka, kstd, kcol, stream_ptr()), "natinf_step_f32prod_inpaint")
                return z_next
            check(lib.natinf_step_f32prod_noise_guided(ptr(z), ptr(cond), ptr(uncond), ptr(cfg), ptr(uncond_slot), int(n_uncond), *tail,
                                                       stream_ptr()), "natinf_step_f32prod_noise_guided")
            return z_next
        check(lib.natinf_step_f32prod_noise(ptr(z), ptr(cond), ptr(uncond), float(cfg), *tail, stream_ptr()), "natinf_step_f32prod_noise")
        return z_next


class SD3NI:
    """Row-normalised fp16 weighted mean + CFG + next flow input (SD3NaturalInference.py:157-168,198-223).

    ``elems_per_image`` pins the per-image size the per-image-guidance form of ``step`` must be called with (None: whatever
    ``sample_elems`` each call gives).  ``step`` takes per-image guidance as ``cfg=<tensor>`` with ``uncond_slot``
    (natinf_step_f16chain_guided); without them it is natinf_step_f16chain with the one ``cfg`` given here.

    Latent-space inpainting (``known=`` / ``mask=`` of the tensor-``cfg`` ``step``, and of ``first_input``; natinf_step_f16chain_inpaint): the known latent
    elements of every ``x_next`` are overwritten, inside the step's launch, with ``sig_next*n + (1 - sig_next)*known`` in the chain's fp16 rounding order
    (``sd_known_schedule``); ``blend_mean`` on the last step puts ``known`` itself into the mean the job returns."""

    def __init__(self, weights: np.ndarray, sigmas: torch.Tensor, n_elem: int, device="cuda:0", cfg: float = 7.0,
                 dense: bool = False, euler: bool = False, elems_per_image: Optional[int] = None):
        _lib.require_gpu()
        if n_elem % 8:
            raise ValueError("element count must be a multiple of 8")
        self.E = int(n_elem)
        self.epi = None if elems_per_image is None else int(elems_per_image)
        _check_elems_per_image(self.epi, self.E, 8)
        self.device = torch.device(device)
        self.cfg = float(cfg)
        self.euler = bool(euler)
        sig = sigmas.detach().to("cpu", torch.float32)
        h = lambda t: float(t.to(torch.float16))                     # 0-d fp32 tensor -> fp16 value, as torch casts it
        if euler:
            # weights w_j = sigma_j - sigma_{j+1} are fp32 0-d tensors: as the FIRST operand of `w * x` eager
            # PyTorch casts them to fp16, but as the SECOND operand of `acc / total` the CPU kernel keeps the
            # fp32 value (original_scalar_value); the row total is the fp32 running sum (SD3...:61-69).
            # This pins eager-CPU semantics (what tests/golden/sd3_form.npz was captured with).  On CUDA the
            # divisor is a 0-d device tensor and the Half functor rounds it to fp16 first: up to 1 fp16 ulp in
            # the mean -- a property of the reference's platform, not of the algorithm; the bit-exact contract
            # of the Euler twin is therefore stated against the CPU run.
            n = sig.numel() - 1
            w32 = [-1 * (sig[i + 1] - sig[i]) for i in range(n)]
            W = np.zeros((n, n))
            tot = []
            for k in range(n):
                acc = 0
                for j in range(k + 1):
                    W[k, j] = h(w32[j])
                    acc = acc + w32[j]
                tot.append(float(acc))
            self.rows = SparseRows(W, lambda k: k + 1, torch.float32, self.device, dense=dense)
            self.totals = tot
        else:
            W = np.asarray(weights, np.float64)
            n = W.shape[0]
            self.rows = SparseRows(W, lambda k: k + 1, torch.float32, self.device, dense=dense)
            self.totals = [r.total for r in self.rows.rows]
        self.n_step = n
        self.sig = [h(sig[k]) for k in range(n + 1)]
        self.oms = [h(1 - sig[k]) for k in range(n + 1)]
        self.hist = torch.empty((n, self.E), dtype=torch.float16, device=self.device)
        self._x = [torch.empty(self.E, dtype=torch.float16, device=self.device) for _ in range(2)]
        self.mean = torch.empty(self.E, dtype=torch.float16, device=self.device)
        self._known_level = _level_memo(lambda renoise: sd_known_schedule(self.sig, self.oms, renoise))

    def _sample_elems(self, sample_elems: Optional[int]) -> int:
        se = self.epi if sample_elems is None else int(sample_elems)
        if se is None or se <= 0 or se % 8 or self.E % se or (self.epi is not None and se != self.epi):
            raise ValueError("sample_elems must be the per-image element count: a multiple of 8 dividing the element count"
                             + ("" if self.epi is None else f" (elems_per_image = {self.epi})"))
        return se

    def first_input(self, noises: torch.Tensor, known: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, *,
                    seed: Optional[int] = None, index=None, renoise: str = "fresh", sample_elems: Optional[int] = None) -> torch.Tensor:
        """x_0 = sigma_0*noise + (1-sigma_0)*0 in fp16 ops (SD3...:207-209 with an empty history).  With ``known`` / ``mask`` (inpainting:
        ``step``'s arguments of those names, with ``seed``, ``index``, ``renoise`` and ``sample_elems``) the known elements of x_0 are the known
        latents at level 0 of ``sd_known_schedule`` (natinf_known_blend_f16); ``noises`` itself is left as it is."""
        n = noises.contiguous().reshape(-1)
        inpaint = known is not None or mask is not None
        if inpaint:                                                  # refusals first: nothing below touches the GPU before them
            se = self._sample_elems(sample_elems)
            ks, ms = check_known_f16(known, mask, self.E, se, seed=seed, renoise=renoise, device=n.device)
            sig, oms, col = self._known_level(0, renoise)
            if n.dtype != torch.float16 or n.numel() != self.E:
                raise ValueError("noises must be an fp16 tensor of n_elem elements")
            index, first, stride = image_index_args(index, self.E // se, n.device)
        if self.euler:
            out = n.clone()                                          # SD3...:94: curr_outputs = deepcopy(noises)
        else:
            out = self._x[1]
            check(lib.natinf_flow_input_f16(ptr(n), None, ptr(out), self.sig[0], self.oms[0], self.E, stream_ptr()),
                  "natinf_flow_input_f16")
        if inpaint:
            check(lib.natinf_known_blend_f16(ptr(out), ptr(out), ptr(n), ptr(known), ptr(mask), ks, ms, sig, oms, col,
                                             0 if seed is None else int(seed) & (2 ** 64 - 1), ptr(index), first, stride, se, self.E,
                                             stream_ptr()), "natinf_known_blend_f16")
        return out

    def step(self, k: int, x: torch.Tensor, v_text: torch.Tensor, v_null: Optional[torch.Tensor], noises: torch.Tensor,
             want_next: bool = True, *, cfg=None, uncond_slot: Optional[torch.Tensor] = None, n_uncond: Optional[int] = None,
             sample_elems: Optional[int] = None, known: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
             seed: Optional[int] = None, index=None, renoise: str = "fresh", blend_mean: bool = False):
        """``cfg`` None: one scale for the launch (the constructor's), ``v_null`` image i belongs to image i.  ``cfg`` a tensor
        (natinf_step_f16chain_guided): the per-image scales, fp32 ``[n]`` on the device, with ``uncond_slot`` int32 ``[n]`` on the
        device -- image i's row in ``v_null``, or -1 for an unguided image (f = x - sig*v_text, its scale is not read); an image is
        ``sample_elems`` elements (default: ``elems_per_image``).  ``v_null`` then holds ``n_uncond`` images, contiguous (default:
        ``v_null.numel() // sample_elems``; None = no row).  The entry reads ``uncond_slot`` back before it launches: fill it
        before the call, once per batch.

        ``known`` / ``mask`` (tensor-``cfg`` form only; natinf_step_f16chain_inpaint): flat fp16 / uint8 device tensors of ``n_elem`` elements (one
        row per image) or ``sample_elems`` elements (one row for every image); a non-zero mask byte marks a known latent element (one byte per
        ELEMENT: a per-cell mask is repeated over the channels by the caller), which leaves the step in ``x_next`` as ``known`` at the step's own
        next level: entry k + 1 of ``sd_known_schedule``.  ``renoise="fresh"`` draws that level's noise from Philox(``seed``, global image index
        ``index`` -- one of ``image_index_args``' forms --, column ``KNOWN_COLUMN0 + k + 1``); ``"same"`` uses ``noises``.  ``blend_mean`` (the last
        step of a job, whose result is the mean): the returned mean holds ``known`` itself at the known elements.  The history never sees either."""
        guided = isinstance(cfg, torch.Tensor)
        inpaint = known is not None or mask is not None
        if not guided and (cfg is not None or uncond_slot is not None or n_uncond is not None or sample_elems is not None):
            raise ValueError("uncond_slot / n_uncond / sample_elems go with a tensor cfg (per-image scales); the launch-wide scale is the constructor's")
        if not guided and inpaint:
            raise ValueError("known / mask go with a tensor cfg (per-image scales): the launch-wide form has no blend")
        if not inpaint and (seed is not None or index is not None or blend_mean):
            raise ValueError("seed / index / blend_mean go with known= and mask=")
        x_next = _pingpong(self._x, k, x)
        idx, val, n = self.rows.ptrs(k)
        r = self.rows.rows[k]
        flags = _lib.SD3_CFG_ON_VELOCITY if self.euler else 0
        if guided:
            se = self._sample_elems(sample_elems)
            m = self.E // se
            if inpaint:                                              # refusals first: nothing below touches the GPU before them
                ks, ms = check_known_f16(known, mask, self.E, se, seed=seed, renoise=renoise, device=x.device)
                _, _, col = self._known_level(k + 1, renoise)
                index, first, stride = image_index_args(index, m, x.device)
            _check_guidance_tensors(cfg, uncond_slot, m, x.device)
            if n_uncond is None:
                n_uncond = 0 if v_null is None else v_null.numel() // se
            # what natinf_step_f16chain_guided and natinf_step_f16chain_inpaint share in front of their flags
            head = (ptr(x), ptr(v_text), ptr(v_null), ptr(cfg), ptr(uncond_slot), int(n_uncond), se, ptr(noises), ptr(self.hist), ptr(self.mean),
                    ptr(x_next) if want_next else None, idx, val, n, r.diag, self.totals[k], k, self.sig[k], self.sig[k + 1], self.oms[k + 1])
            if inpaint:
                check(lib.natinf_step_f16chain_inpaint(*head, flags | (_lib.SD3_BLEND_MEAN if blend_mean else 0), self.E, ptr(known), ptr(mask),
                                                       ks, ms, col, 0 if seed is None else int(seed) & (2 ** 64 - 1), ptr(index), first, stride,
                                                       stream_ptr()), "natinf_step_f16chain_inpaint")
                return self.mean, (x_next if want_next else None)
            check(lib.natinf_step_f16chain_guided(*head, flags, self.E, stream_ptr()), "natinf_step_f16chain_guided")
            return self.mean, (x_next if want_next else None)
        check(lib.natinf_step_f16chain(ptr(x), ptr(v_text), ptr(v_null), ptr(noises), ptr(self.hist), ptr(self.mean),
                                       ptr(x_next) if want_next else None, idx, val, n, r.diag, self.totals[k], k,
                                       self.sig[k], self.sig[k + 1], self.oms[k + 1], self.cfg, flags, self.E,
                                       stream_ptr()), "natinf_step_f16chain")
        return self.mean, (x_next if want_next else None)
