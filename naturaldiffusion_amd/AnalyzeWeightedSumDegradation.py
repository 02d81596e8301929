"""src/AnalyzeWeightedSumDegradation.py on gfx950: ``get_feature``, the script's encoder call
(``vae.encode(images).latent_dist.sample().mul_(0.18215)``, :37-60), on the AutoencoderKL encoder engine, and the posterior-concentration
statistics of ``get_vp_statistics_tx`` / ``get_flow_statistics_tx`` (:93-227) on the posterior kernels (include/natinf_posterior.h).

Reading the files and the ADM centre crop (:16-45) stay with the caller, who hands over the cropped pictures as one uint8
array; so does loading the per-class ``.pt`` feature files (:135, :193), which ``get_statistics`` takes as tensors or as callables that return one.

``get_feature``.  What changes against the reference: the posterior noise of an image is keyed by (seed, global image index) instead of coming
from one sequential ``torch.randn`` stream, so the latents do not depend on the batch size or on how many ranks share the job (shard.rank_batches).
The encoder comes from ``ValidateNaturalInference.load_vae_encoder(vae_path)`` (the weights file ``load_vae_decoder`` reads) or from ``vae.VAEEncoder`` directly.

``posterior_stats`` / ``get_statistics``.  Per class and noise level the script noises every feature vector, takes all squared distances to the
clean vectors with an fp32 ``torch.cdist``, and reads ``p_ii`` and ``max_j p_ij`` off an fp64 row softmax.  Here the row-constant ``|s_i|^2`` is
dropped (it cancels in the softmax), ``s_i . f_j`` is three exact bf16 MFMA passes over the split ``s = hi + mid + lo`` with the fp32 accumulators
added into fp64 every 512 values of k, and everything after the GEMM is fp64 (measured error and time in
profiles/posterior/).  The samples themselves are the reference's bytes (``feats * a + noise * b`` in fp32) when the caller passes the
reference's noise; by default the noise of row r of class c is Philox keyed by (seed, (c << 20) + r), so a class's statistics do not depend on
the rank that computes it or on the other classes of the job.  The host statements (:148-165) are ``summarize``.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .shard import rank_batches, rank_indices


def preprocess(images_u8: torch.Tensor, flip: bool = False) -> torch.Tensor:
    """[n, H, W, 3] uint8 -> [n, 3, H, W] fp32 in [-1, 1]: ``(x / 255 - 0.5) / 0.5`` (:47-49), after the optional left-right flip (:43)."""
    x = images_u8.flip(2) if flip else images_u8
    x = (x.to(torch.float32) / 255 - 0.5) / 0.5
    return x.permute(0, 3, 1, 2).contiguous()


def get_feature(encoder, images_u8, flip: bool = False, batch_size: int = 16, rank: int = 0, world: int = 1, seed: int = 0,
                scale: float = 0.18215) -> Tuple[torch.Tensor, torch.Tensor]:
    """Latents of this rank's share of ``images_u8`` ([N, H, W, 3] uint8, already cropped to the encoder's size): returns
    (latents [n, C, r, r] fp32 on the CPU, their global indices [n] int64).  Image i is encoded with global index i."""
    if isinstance(images_u8, np.ndarray):
        images_u8 = torch.from_numpy(np.ascontiguousarray(images_u8))
    if images_u8.dim() != 4 or images_u8.shape[3] != 3 or images_u8.dtype != torch.uint8:
        raise ValueError("images_u8 must be [N, H, W, 3] uint8")
    if batch_size < 1 or batch_size > encoder.max_batch:
        raise ValueError(f"batch_size must be in 1..{encoder.max_batch} (the encoder's max_batch)")
    feats, index = [], []
    for batch in rank_batches(int(images_u8.shape[0]), batch_size, rank, world):
        idx = torch.tensor(batch, dtype=torch.int64)
        x = preprocess(images_u8[idx], flip)
        z = encoder.encode(x.to(encoder.device), sample=True, scale=scale, shift=0.0, seed=seed, index=idx)
        feats.append(z.cpu())
        index.append(idx)
    if not feats:
        r = encoder.latent_res
        return torch.empty((0, encoder.latent_ch, r, r), dtype=torch.float32), torch.empty((0,), dtype=torch.int64)
    return torch.cat(feats), torch.cat(index)


# ---- the statistics (:93-227) ----

TS = (200, 300, 400, 500, 600, 700, 800, 900)          # the noise levels of both loops (:127, :185)
CLASS_SHIFT = 20                                         # global index of row r of class c: (c << 20) + r
MAX_N, MAX_D = 4096, 65536                               # include/natinf_posterior.h


def vp_schedule() -> Tuple[np.ndarray, np.ndarray]:
    """(alphas_bar, sigmas), fp64 [1000]: the reference's statements (:113-116)."""
    betas = np.linspace(0.0001, 0.02, 1000, dtype=np.float64)
    alphas = 1 - betas
    alphas_bar = np.cumprod(alphas)
    sigmas = np.sqrt((1 - alphas_bar) / alphas_bar)
    return alphas_bar, sigmas


def flow_schedule() -> Tuple[np.ndarray, np.ndarray]:
    """(data_scales, sigmas), fp64 [1000]: the reference's statements (:174-175)."""
    data_scales = np.linspace(1, 0.00001, 1000, dtype=np.float64)
    sigmas = (1 - data_scales) / data_scales
    return data_scales, sigmas


def level_scalars(form: str, t: int) -> Tuple[float, float, float]:
    """(a, b, sigma) of noise level t: samples = feats * a + noise * b (:98, :107).  a and b are rounded to fp32, as torch rounds a
    Python scalar that meets an fp32 tensor; sigma stays fp64."""
    if form == "vp":
        ab, sig = vp_schedule()
        a, b = np.sqrt(ab[t]), np.sqrt(1 - ab[t])
    elif form == "flow":
        ds, sig = flow_schedule()
        a, b = ds[t], 1 - ds[t]
    else:
        raise ValueError("form must be 'vp' or 'flow'")
    return float(np.float32(a)), float(np.float32(b)), float(sig[t])


def _as_bf16_rows(feats: torch.Tensor) -> torch.Tensor:
    """[n, ...] -> [n, d] bf16, refusing what the cast would change"""
    if not isinstance(feats, torch.Tensor) or feats.dim() < 2:
        raise ValueError("feats must be a tensor [n, ...]")
    f = feats.reshape(feats.shape[0], -1)
    if f.dtype == torch.float32:
        fb = f.to(torch.bfloat16)
        if not torch.equal(fb.to(torch.float32), f):
            raise ValueError("feats holds fp32 values that bf16 cannot represent: cast them as the reference does before it saves "
                             "them, feats.to(dtype=torch.bfloat16) (src/AnalyzeWeightedSumDegradation.py:87)")
        f = fb
    elif f.dtype != torch.bfloat16:
        raise ValueError("feats must be bf16, or fp32 holding bf16 values: cast them as the reference does before it saves them, "
                         "feats.to(dtype=torch.bfloat16) (src/AnalyzeWeightedSumDegradation.py:87)")
    n, d = int(f.shape[0]), int(f.shape[1])
    if n < 1 or n > MAX_N or d < 64 or d > MAX_D or d % 64:
        raise ValueError(f"feats [n, d] = [{n}, {d}]: n must be in 1..{MAX_N} and d a multiple of 64 in 64..{MAX_D}")
    return f.contiguous()


class PosteriorSamples:
    """The noised samples of one class on the device, split into the three bf16 planes of the GEMM: ``stats(sigma)`` may be called any number
    of times.  ``noise`` ([n, d] fp32) or Philox keyed by (seed, index[i]); see ``posterior_stats``."""

    def __init__(self, feats: torch.Tensor, a: float, b: float, *, seed: int = 0, index: Optional[torch.Tensor] = None,
                 noise: Optional[torch.Tensor] = None, device=None):
        from . import _lib
        f = _as_bf16_rows(feats)
        self.n, self.d = int(f.shape[0]), int(f.shape[1])
        if noise is not None:
            if noise.dtype != torch.float32 or noise.numel() != f.numel():
                raise ValueError("noise must be fp32 with as many values as feats")
            noise = noise.reshape(self.n, self.d)
        elif index is None:
            index = torch.arange(self.n, dtype=torch.int64)
        elif index.dtype != torch.int64 or tuple(index.shape) != (self.n,):
            raise ValueError("index must be int64 [n]")
        _lib.require_gpu()
        self.device = torch.device(device if device is not None else "cuda")
        self._lib = _lib
        self.feats = f.to(self.device)
        nbytes = _lib.lib.natinf_posterior_workspace_bytes(self.n, self.d)
        _lib.check(min(nbytes, 0), "natinf_posterior_workspace_bytes")
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        eps = None if noise is None else noise.to(self.device).contiguous()
        idx = None if noise is not None else index.to(self.device).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.natinf_posterior_samples(_lib.ptr(self.feats), _lib.ptr(eps), float(a), float(b), int(seed) & (2 ** 64 - 1),
                                                         _lib.ptr(idx), 0, 1, self.n, self.d, _lib.ptr(self._ws), _lib.stream_ptr()),
                       "natinf_posterior_samples")
            torch.cuda.current_stream().synchronize()            # eps / idx may go once the kernel has read them

    def stats(self, sigma: float) -> Tuple[torch.Tensor, torch.Tensor]:
        """(p_diag, p_max): fp64 CPU tensors [n]"""
        if not (sigma > 0 and np.isfinite(sigma)):
            raise ValueError("sigma must be positive and finite")
        L = self._lib
        out = torch.empty((2, self.n), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib.natinf_posterior_stats(L.ptr(self.feats), float(sigma), self.n, self.d, L.ptr(self._ws), L.ptr(out[0]), L.ptr(out[1]),
                                                 L.stream_ptr()), "natinf_posterior_stats")
        out = out.cpu()
        return out[0].clone(), out[1].clone()

    def samples(self) -> torch.Tensor:
        """hi + mid + lo of the planes: the fp32 samples [n, d] on the CPU (natinf_posterior_debug_planes; for tests)"""
        L = self._lib
        s = torch.empty((self.n, self.d), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            L.check(L.lib.natinf_posterior_debug_planes(L.ptr(self._ws), self.n, self.d, L.ptr(s)), "natinf_posterior_debug_planes")
        return s.cpu()


def posterior_stats(feats: torch.Tensor, a: float, b: float, sigma: float, *, seed: int = 0, index: Optional[torch.Tensor] = None,
                    noise: Optional[torch.Tensor] = None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(p_diag, p_max), fp64 CPU tensors [n], of one class at one noise level: with s_i = feats_i * a + eps_i * b in fp32 and
    p_ij = softmax_j(-|s_i - feats_j|^2 / (2 sigma^2)) in fp64, p_diag[i] = p_ii and p_max[i] = max_j p_ij (:139-146).

    ``feats`` is [n, ...] (flattened to [n, d]; n <= 4096, d a multiple of 64 up to 65536), bf16 or fp32 holding bf16 values.  ``noise`` is an
    fp32 tensor of feats' size for a caller who wants the reference's ``torch.Generator`` stream (:94-97); with ``noise=None`` eps_i is Philox keyed
    by (seed, index[i]) -- ``index`` int64 [n], default arange(n) -- the values ``natinf_randn_philox_f32`` returns."""
    return PosteriorSamples(feats, a, b, seed=seed, index=index, noise=noise, device=device).stats(sigma)


def summarize(p_diag, p_max) -> Dict[str, object]:
    """The reference's host statements for one class (:148-165): x0_count = how many p_ii exceed 0.9, xx_count = the sum of the row maxima, and
    the two 100-bin histograms over [0, 1]."""
    p_diag, p_max = torch.as_tensor(p_diag), torch.as_tensor(p_max)
    x0_count = (p_diag > 0.9).sum().item()
    xx_count = p_max.sum().item()
    hist_x0, _ = np.histogram(p_diag.cpu().numpy(), bins=100, range=(0, 1))
    hist_xx, _ = np.histogram(p_max.cpu().numpy(), bins=100, range=(0, 1))
    return dict(x0_count=x0_count, xx_count=xx_count, hist_x0=hist_x0, hist_xx=hist_xx, n=int(p_max.shape[0]))


def get_statistics(class_feats: Sequence[Union[torch.Tensor, Callable[[], torch.Tensor]]], form: str = "vp", ts: Sequence[int] = TS,
                   seed: int = 0, rank: int = 0, world: int = 1, device=None) -> Dict[int, Dict[str, object]]:
    """get_vp_statistics_tx / get_flow_statistics_tx (:111-169, :172-227) over this rank's classes: class c belongs to rank c % world.
    Row r of class c draws its noise with global index (c << 20) + r, the same at every level (the reference reuses a class's seed at every t too).

    Returns {t: dict(hist_x0, hist_xx [100] int64, classes [k], x0_counts [k], xx_counts [k], total_count)} with one entry per class of this
    rank, in class order.  Ranks' results are added with ``merge_statistics``; the reference's printed ratios are x0_counts.sum() / total_count
    and xx_counts.sum() / total_count."""
    ts = [int(t) for t in ts]
    levels = {t: level_scalars(form, t) for t in ts}
    out = {t: dict(hist_x0=np.zeros(100, dtype=np.int64), hist_xx=np.zeros(100, dtype=np.int64), classes=[], x0_counts=[], xx_counts=[],
                   total_count=0) for t in ts}
    for c in rank_indices(len(class_feats), rank, world):
        feats = class_feats[c]
        if callable(feats):
            feats = feats()
        n = int(feats.shape[0])
        if n >= 1 << CLASS_SHIFT:
            raise ValueError("a class holds at most 2^20 rows")
        index = (c << CLASS_SHIFT) + torch.arange(n, dtype=torch.int64)
        for t in ts:
            a, b, sigma = levels[t]
            s = summarize(*posterior_stats(feats, a, b, sigma, seed=seed, index=index, device=device))
            o = out[t]
            o["hist_x0"] += s["hist_x0"]
            o["hist_xx"] += s["hist_xx"]
            o["classes"].append(c)
            o["x0_counts"].append(s["x0_count"])
            o["xx_counts"].append(s["xx_count"])
            o["total_count"] += s["n"]
    return out


def merge_statistics(parts: Sequence[Dict[int, Dict[str, object]]]) -> Dict[int, Dict[str, object]]:
    """Add the results of several ranks (``get_statistics``): histograms and total_count summed, the per-class lists joined in class order."""
    out = {}
    for t in parts[0]:
        rows = sorted((c, x0, xx) for p in parts for c, x0, xx in zip(p[t]["classes"], p[t]["x0_counts"], p[t]["xx_counts"]))
        out[t] = dict(hist_x0=sum(p[t]["hist_x0"] for p in parts), hist_xx=sum(p[t]["hist_xx"] for p in parts),
                      classes=[r[0] for r in rows], x0_counts=[r[1] for r in rows], xx_counts=[r[2] for r in rows],
                      total_count=sum(p[t]["total_count"] for p in parts))
    return out
