"""src/AnalyzeWeightedSumDegradation.py on the gfx950 encoder engine: ``get_feature``, the script's one GPU call
(``vae.encode(images).latent_dist.sample().mul_(0.18215)``, :37-60).

Reading the files and the ADM centre crop (:16-45) stay with the caller, who hands over the cropped pictures as one uint8
array; the ``cdist`` statistics of the script (:111-) are not part of this module.  What changes against the reference: the
posterior noise of an image is keyed by (seed, global image index) instead of coming from one sequential ``torch.randn``
stream, so the latents do not depend on the batch size or on how many ranks share the job (shard.rank_batches).  The encoder comes from
``ValidateNaturalInference.load_vae_encoder(vae_path)`` (the weights file ``load_vae_decoder`` reads) or from ``vae.VAEEncoder`` directly.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from .shard import rank_batches


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
