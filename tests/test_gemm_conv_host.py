"""CPU check of the reference that tests/test_gpu_gemm_conv.py holds the implicit-convolution GEMMs to: the zero-bordered operand, the
packed weights in the engine's K order and the nine-shift fp64 sum give F.conv2d (+ the 1x1 shortcut), on any machine."""
import importlib.util
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

_spec = importlib.util.spec_from_file_location("_gemm_conv_helpers", Path(__file__).with_name("test_gpu_gemm_conv.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)


@pytest.mark.parametrize("B,res,cin,N,c1", [(3, 4, 64, 8, 0), (2, 8, 128, 16, 64), (1, 16, 64, 24, 32), (5, 2, 192, 8, 0)])
def test_nine_shift_reference_matches_conv2d(B, res, cin, N, c1):
    g = torch.Generator().manual_seed(B * res + cin)
    x = torch.randn(B, cin, res, res, generator=g, dtype=torch.float64)
    w = torch.randn(N, cin, 3, 3, generator=g, dtype=torch.float64)
    s = torch.randn(B, c1, res, res, generator=g, dtype=torch.float64) if c1 else None
    w1 = torch.randn(N, c1, generator=g, dtype=torch.float64) if c1 else None
    bias = torch.randn(N, generator=g, dtype=torch.float64)
    a_pad = H.pad_nhwc(x)
    assert a_pad.shape == (B, res + 2, res + 2, cin)
    assert (a_pad[:, 0] == 0).all() and (a_pad[:, -1] == 0).all() and (a_pad[:, :, 0] == 0).all() and (a_pad[:, :, -1] == 0).all()
    wp = H.pack_weights(w, w1)
    assert wp.shape == (N, 9 * cin + c1)
    # the K order itself: column ((c / 64) * 9 + 3 ky + kx) * 64 + c % 64 holds w[n, c, ky, kx]
    for c, ky, kx in ((0, 0, 0), (cin - 1, 2, 2), (min(70, cin - 1), 1, 2), (63, 2, 0)):
        assert torch.equal(wp[:, ((c // 64) * 9 + 3 * ky + kx) * 64 + c % 64], w[:, c, ky, kx])
    a1 = s.permute(0, 2, 3, 1).reshape(-1, c1) if c1 else None
    got = H.conv_ref(a_pad, wp, a1, bias, 0.5)
    ref = F.conv2d(x, w, bias, padding=1)
    if c1:
        ref = ref + torch.einsum("bkhw,nk->bnhw", s, w1)
    ref = (ref * 0.5).permute(0, 2, 3, 1).reshape(-1, N)
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)
