"""Oracle: AutoencoderKL ENCODER forward + ``quant_conv`` (the moments ``vae.encode`` of src/AnalyzeWeightedSumDegradation.py:56 builds its
``DiagonalGaussianDistribution`` from), torch CPU fp32.  Not a test module: the encoder tests import it as a sibling.

TEST INFRASTRUCTURE ONLY.

**PARITY UNPINNED.**  The reference takes this module from ``diffusers`` (``AutoencoderKL.from_pretrained``) -- un-vendored, un-pinned, and no
test or fixture of the reference touches its arithmetic (see the header of oracle/vae_oracle.py).  This file restates the published architecture
of the encoder (Rombach et al. 2022 first-stage model; diffusers' ``Encoder`` module layout and state-dict key names):

  conv_in 3x3 (3 -> 128); down_blocks 0..3 with 2 ResnetBlocks each (channels 128, 256, 512, 512; a 1x1 ``conv_shortcut`` where the channel
  count changes) and, after blocks 0..2, a 3x3 stride-2 convolution over the input padded by one zero row / column at the bottom / right
  (``Downsample2D(padding=0)`` after ``F.pad(x, (0, 1, 0, 1))``); mid_block: ResnetBlock, single-head self-attention, ResnetBlock;
  conv_norm_out (GroupNorm) -> SiLU -> conv_out 3x3 (512 -> 2 * latent_ch); then AutoencoderKL's 1x1 ``quant_conv`` when the model has one.
The ResnetBlock, GroupNorm and attention arithmetic are the decoder oracle's, imported from it.
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from oracle.vae_oracle import _attn, _gn, _res

CH = (128, 256, 512, 512)          # block_out_channels


def param_shapes(latent_ch: int = 4) -> Dict[str, tuple]:
    s: Dict[str, tuple] = {"conv_in.weight": (128, 3, 3, 3), "conv_in.bias": (128,)}

    def res(p, cin, cout):
        s[p + "norm1.weight"] = (cin,); s[p + "norm1.bias"] = (cin,)
        s[p + "conv1.weight"] = (cout, cin, 3, 3); s[p + "conv1.bias"] = (cout,)
        s[p + "norm2.weight"] = (cout,); s[p + "norm2.bias"] = (cout,)
        s[p + "conv2.weight"] = (cout, cout, 3, 3); s[p + "conv2.bias"] = (cout,)
        if cin != cout:
            s[p + "conv_shortcut.weight"] = (cout, cin, 1, 1); s[p + "conv_shortcut.bias"] = (cout,)
    cin = 128
    for i, cout in enumerate(CH):
        for j in range(2):
            res(f"down_blocks.{i}.resnets.{j}.", cin if j == 0 else cout, cout)
        if i < 3:
            s[f"down_blocks.{i}.downsamplers.0.conv.weight"] = (cout, cout, 3, 3); s[f"down_blocks.{i}.downsamplers.0.conv.bias"] = (cout,)
        cin = cout
    res("mid_block.resnets.0.", 512, 512)
    a = "mid_block.attentions.0."
    s[a + "group_norm.weight"] = (512,); s[a + "group_norm.bias"] = (512,)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        s[a + n + ".weight"] = (512, 512); s[a + n + ".bias"] = (512,)
    res("mid_block.resnets.1.", 512, 512)
    s["conv_norm_out.weight"] = (512,); s["conv_norm_out.bias"] = (512,)
    s["conv_out.weight"] = (2 * latent_ch, 512, 3, 3); s["conv_out.bias"] = (2 * latent_ch,)
    return s


def make_params(latent_ch: int = 4, seed: int = 0) -> Dict[str, torch.Tensor]:
    """The decoder oracle's recipe: fan-in-scaled uniform filters / matrices, norm scales 1 + 0.1 N(0,1), biases 0.02 N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shp in param_shapes(latent_ch).items():
        if len(shp) >= 2:
            lim = math.sqrt(3.0 / int(np.prod(shp[1:])))
            out[name] = (torch.rand(shp, generator=g) * 2 - 1) * lim
        elif "norm" in name and name.endswith("weight"):
            out[name] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        else:
            out[name] = 0.02 * torch.randn(shp, generator=g)
    return out


@torch.no_grad()
def encode_moments(P: Dict[str, torch.Tensor], images: torch.Tensor) -> torch.Tensor:
    """images [B, 3, 8r, 8r] -> moments [B, 2 * latent_ch, r, r] = quant_conv(encoder(images)): mean channels, then logvar."""
    x = F.conv2d(images.float(), P["conv_in.weight"], P["conv_in.bias"], padding=1)
    for i in range(4):
        for j in range(2):
            x = _res(P, f"down_blocks.{i}.resnets.{j}.", x)
        if i < 3:
            p = f"down_blocks.{i}.downsamplers.0.conv."
            x = F.conv2d(F.pad(x, (0, 1, 0, 1)), P[p + "weight"], P[p + "bias"], stride=2)
    x = _res(P, "mid_block.resnets.0.", x)
    x = _attn(P, "mid_block.attentions.0.", x)
    x = _res(P, "mid_block.resnets.1.", x)
    x = F.conv2d(F.silu(_gn(P, "conv_norm_out", x)), P["conv_out.weight"], P["conv_out.bias"], padding=1)
    if "quant_conv.weight" in P:                         # AutoencoderKL.encode: moments = quant_conv(encoder(x))
        n2 = x.shape[1]
        x = F.conv2d(x, P["quant_conv.weight"].reshape(n2, n2, 1, 1), P["quant_conv.bias"])
    return x
