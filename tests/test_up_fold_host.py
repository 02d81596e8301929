"""The identity behind natinf_set_fuse_up_fold: a 3x3 convolution over a 2x nearest-up-sampled image IS four 2x2 convolutions over the low-resolution image, one per
output parity (a, b), with the row / column sums of the 3x3 kernel as weights; zero padding carries over (output row -1 is input row -1, output row 2 R is input row R).
float64, no GPU: this pins the tap / parity / border mapping that k_fold_up_conv and the up-fold launch (csrc/gemm_dma.h, UPW) implement."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from up_fold_mirror import fold_up_numpy


@pytest.mark.parametrize("res", [4, 8])
def test_four_phase_convolutions_equal_the_convolution_of_the_up_sampled_image(res):
    g = torch.Generator().manual_seed(res)
    cin, cout = 3, 2
    h = torch.randn(2, cin, res, res, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(h, scale_factor=2, mode="nearest"), w, padding=1)
    wp = torch.from_numpy(fold_up_numpy(w.numpy()))                     # [a][b][cout][cin][ty][tx]
    got = torch.zeros_like(ref)
    hp = F.pad(h, (1, 1, 1, 1))                                         # input pixel (y, x) at hp[y + 1, x + 1]
    for a in (0, 1):
        for b in (0, 1):
            # output (2 i + a, 2 j + b) = sum_{ty, tx} Wp[a][b][ty][tx] * h[i + a - 1 + ty, j + b - 1 + tx]: a valid 2x2 correlation of the padded window starting at (a, b)
            win = hp[:, :, a:a + res + 1, b:b + res + 1]
            got[:, :, a::2, b::2] = F.conv2d(win, wp[a, b])
    assert (got - ref).abs().max().item() <= 1e-12


def test_mirror_keeps_the_documented_summation_order():
    """rows first, then columns, each pair as (W[lo] + W[hi]) -- in float32 the order is visible"""
    w = np.random.default_rng(0).standard_normal((1, 1, 3, 3)).astype(np.float32)
    wp = fold_up_numpy(w)
    k = w[0, 0]
    assert wp[0, 0, 0, 0, 1, 1] == (k[1, 1] + k[2, 1]) + (k[1, 2] + k[2, 2])
    assert wp[1, 1, 0, 0, 0, 0] == (k[0, 0] + k[1, 0]) + (k[0, 1] + k[1, 1])
    assert wp[0, 1, 0, 0, 0, 1] == k[0, 2] and wp[1, 0, 0, 0, 1, 0] == k[2, 0]
    assert wp[0, 0, 0, 0, 0, 1] == k[0, 1] + k[0, 2] and wp[1, 1, 0, 0, 0, 1] == k[0, 2] + k[1, 2]
