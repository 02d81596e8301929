"""Oracle of the posterior statistics (src/AnalyzeWeightedSumDegradation.py:93-108, 139-146), torch CPU.  Not a test module: the posterior tests
import it as a sibling.

TEST INFRASTRUCTURE ONLY.

  * ``reference_stats``  the reference's statements, fp32 ``torch.cdist`` and all
  * ``exact_stats``      the same quantities in fp64 throughout
  * ``competing_feats``  the input recipe of the accuracy tests: rows close enough to compete for the posterior mass
"""
from __future__ import annotations

import numpy as np
import torch


def add_noise(feats_f32: torch.Tensor, noise: torch.Tensor, a: float, b: float) -> torch.Tensor:
    """``samples * np.sqrt(alphas_bar[t]) + noises * np.sqrt(1 - alphas_bar[t])`` (:98) / ``samples * data_scales[t] + noises * (1 - data_scales[t])``
    (:107): fp32 tensors against Python scalars, three fp32 roundings."""
    return feats_f32 * a + noise * b


def reference_stats(samples: torch.Tensor, feats_f32: torch.Tensor, sigma: float):
    """(p_diag, p_max) fp64 [n] by the reference's statements (:139-146)."""
    exponent = -1 * torch.cdist(samples, feats_f32, p=2) ** 2 / (2 * sigma ** 2)
    max_vals = exponent.max(axis=1, keepdim=True)[0]
    ref_dists = (exponent - max_vals).to(dtype=torch.float64)
    exp_vals = torch.exp(ref_dists, out=ref_dists)
    sum_exp_vals = torch.sum(exp_vals, 1, keepdim=True)
    probs = exp_vals / sum_exp_vals
    return probs.diag().clone(), probs.max(axis=1)[0]


def exact_stats(samples: torch.Tensor, feats_f32: torch.Tensor, sigma: float):
    """(p_diag, p_max) fp64 [n] of the same fp32 samples with every later operation in fp64 (the squared distances as explicit differences)."""
    s, f = samples.to(torch.float64), feats_f32.to(torch.float64)
    d2 = torch.empty((s.shape[0], f.shape[0]), dtype=torch.float64)
    for i in range(s.shape[0]):
        d2[i] = ((s[i][None, :] - f) ** 2).sum(1)
    e = -d2 / (2 * sigma ** 2)
    e = e - e.max(1, keepdim=True)[0]
    p = torch.exp(e)
    p = p / p.sum(1, keepdim=True)
    return p.diag().clone(), p.max(1)[0]


def competing_feats(n: int, d: int, b: float, seed: int) -> torch.Tensor:
    """bf16 [n, d]: ``bf16(c + delta * g_j)`` with c, g_j standard normal and delta = 1.5 * b / sqrt(d), b = sqrt(1 - ab_t) (the noise's scale):
    neighbours are about as far apart as the noise moves a sample along their difference, so several rows share the posterior."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(1, d, generator=g, dtype=torch.float64)
    gj = torch.randn(n, d, generator=g, dtype=torch.float64)
    return (c + (1.5 * b / np.sqrt(d)) * gj).to(torch.float32).to(torch.bfloat16)


def rms(x: torch.Tensor) -> float:
    return float(torch.sqrt((x.to(torch.float64) ** 2).mean()))
