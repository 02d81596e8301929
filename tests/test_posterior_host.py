"""Host side of the posterior statistics (include/natinf_posterior.h; naturaldiffusion_amd/AnalyzeWeightedSumDegradation.py): argument checks, the
workspace query, the reference's host statements, the schedules, the sharding of ``get_statistics`` and the bf16 check.  No GPU."""

import numpy as np
import pytest
import torch

from naturaldiffusion_amd import AnalyzeWeightedSumDegradation as A
from naturaldiffusion_amd import _lib

EINVAL = -1
L = _lib.lib

# never dereferenced: every call below must be refused before anything is configured or launched
P = 0x1000            # 256-byte aligned, non-null


def _samples(feats=P, noise=None, n=4, d=64, ws=P):
    return L.natinf_posterior_samples(feats, noise, 1.0, 1.0, 0, None, 0, 1, n, d, ws, None)


def _stats(feats=P, sigma=1.0, n=4, d=64, ws=P, pd=P, pm=P):
    return L.natinf_posterior_stats(feats, sigma, n, d, ws, pd, pm, None)


def _planes(ws=P, n=4, d=64, out=P):
    return L.natinf_posterior_debug_planes(ws, n, d, out)


BAD_SHAPES = [(0, 64), (-1, 64), (4097, 64), (4, 0), (4, 32), (4, 96), (4, 65600), (4, 65536 + 64), (4, -64)]


def test_argument_errors_are_einval():
    for n, d in BAD_SHAPES:
        assert _samples(n=n, d=d) == EINVAL, (n, d)
        assert _stats(n=n, d=d) == EINVAL, (n, d)
        assert _planes(n=n, d=d) == EINVAL, (n, d)
        assert L.natinf_posterior_workspace_bytes(n, d) < 0, (n, d)
    assert _samples(feats=None) == EINVAL and _samples(ws=None) == EINVAL
    assert _samples(feats=P + 2) == EINVAL and _samples(noise=P + 4) == EINVAL and _samples(ws=P + 16) == EINVAL      # 16-byte accesses
    assert _stats(feats=None) == EINVAL and _stats(ws=None) == EINVAL and _stats(pd=None) == EINVAL and _stats(pm=None) == EINVAL
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        assert _stats(sigma=sigma) == EINVAL, sigma
    assert _planes(ws=None) == EINVAL and _planes(out=None) == EINVAL


def test_workspace_bytes_is_monotone():
    ns = [1, 2, 37, 64, 65, 128, 129, 257, 600, 1300, 2200, 4095, 4096]
    ds = [64, 128, 192, 1024, 4096, 16384, 65536]
    b = np.array([[L.natinf_posterior_workspace_bytes(n, d) for d in ds] for n in ns], dtype=np.int64)
    assert (b > 0).all()
    assert (np.diff(b, axis=0) >= 0).all() and (np.diff(b, axis=1) >= 0).all()
    for i, n in enumerate(ns):                        # room for the planes and the norms at least
        for j, d in enumerate(ds):
            assert b[i, j] >= 6 * n * d + 8 * n + 8 * n * n


def _reference_summary(p_diag, p_max):
    """src/AnalyzeWeightedSumDegradation.py:148-165 for one class"""
    x0_count = (p_diag > 0.9).sum().item()
    xx_count = p_max.sum().item()
    hist_x0, _ = np.histogram(p_diag.cpu().numpy(), bins=100, range=(0, 1))
    hist_xx, _ = np.histogram(p_max.cpu().numpy(), bins=100, range=(0, 1))
    return x0_count, xx_count, hist_x0, hist_xx


def test_summarize_is_the_references_host_statements():
    p_diag = torch.tensor([0.0, 0.9, np.nextafter(0.9, 1.0), 0.01, 0.5, 0.99, 1.0, 0.1, 0.3, 0.899999], dtype=torch.float64)
    p_max = torch.tensor([0.02, 0.9, 0.95, 0.01, 0.5, 0.99, 1.0, 0.25, 0.3, 0.91], dtype=torch.float64)
    s = A.summarize(p_diag, p_max)
    x0, xx, h0, hx = _reference_summary(p_diag, p_max)
    assert s["x0_count"] == x0 == 3 and s["xx_count"] == xx and s["n"] == 10            # 0.9 itself does not count (`> 0.9`)
    assert np.array_equal(s["hist_x0"], h0) and np.array_equal(s["hist_xx"], hx)
    assert s["hist_x0"].sum() == 10 and s["hist_x0"][99] == 2 and s["hist_x0"][0] == 1      # 1.0 falls into the last bin, 0.0 into the first


def test_schedules_are_the_references_arrays():
    betas = np.linspace(0.0001, 0.02, 1000, dtype=np.float64)
    alphas_bar = np.cumprod(1 - betas)
    ab, sig = A.vp_schedule()
    assert np.array_equal(ab, alphas_bar) and np.array_equal(sig, np.sqrt((1 - alphas_bar) / alphas_bar))
    data_scales = np.linspace(1, 0.00001, 1000, dtype=np.float64)
    ds, sig = A.flow_schedule()
    assert np.array_equal(ds, data_scales) and np.array_equal(sig[1:], ((1 - data_scales) / data_scales)[1:])
    # a, b: what torch makes of the Python scalar against an fp32 tensor
    x = torch.tensor([1.2345678, -0.333], dtype=torch.float32)
    for form, t in (("vp", 200), ("flow", 300), ("vp", 900)):
        a, b, sigma = A.level_scalars(form, t)
        sa, sb = (np.sqrt(ab[t]), np.sqrt(1 - ab[t])) if form == "vp" else (ds[t], 1 - ds[t])
        assert torch.equal(x * a, x * sa) and torch.equal(x * b, x * sb)
        assert sigma == (A.vp_schedule() if form == "vp" else A.flow_schedule())[1][t]
    with pytest.raises(ValueError):
        A.level_scalars("ve", 200)


def test_bf16_check_rejects_one_stray_mantissa_bit():
    f = torch.randn(4, 64, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    assert A._as_bf16_rows(f).dtype == torch.bfloat16
    assert torch.equal(A._as_bf16_rows(f.float().reshape(4, 4, 16)), f)               # fp32 holding bf16 values, flattened
    bad = f.float().clone()
    bad.view(torch.int32)[2, 5] |= 1 << 15                                            # the first bit bf16 drops
    with pytest.raises(ValueError, match="bfloat16"):
        A._as_bf16_rows(bad)
    with pytest.raises(ValueError, match="bfloat16"):
        A._as_bf16_rows(f.to(torch.float16))
    with pytest.raises(ValueError):
        A._as_bf16_rows(torch.zeros(4, 96, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        A._as_bf16_rows(torch.zeros(4097, 64, dtype=torch.bfloat16))


def test_get_statistics_sharding(monkeypatch):
    """ranks 0 and 1 of world 2, merged, equal world 1; class c is seen with the indices (c << 20) + r whichever rank runs it"""
    seen = []

    def stub(feats, a, b, sigma, *, seed=0, index=None, noise=None, device=None):
        seen.append((int(feats.shape[0]), index.clone(), a, b, sigma, seed))
        g = torch.Generator().manual_seed(int(index[0]) % 1000 + int(sigma * 1000))
        p_max = torch.rand(feats.shape[0], generator=g, dtype=torch.float64)
        return p_max * torch.rand(feats.shape[0], generator=g, dtype=torch.float64), p_max

    monkeypatch.setattr(A, "posterior_stats", stub)
    sizes = [5, 9, 3, 7, 2]
    loaded = []

    def lazy(c):
        def load():
            loaded.append(c)
            return torch.zeros(sizes[c], 64, dtype=torch.bfloat16)
        return load

    classes = [lazy(c) if c % 2 else torch.zeros(sizes[c], 64, dtype=torch.bfloat16) for c in range(5)]
    ts = (200, 900)
    whole = A.get_statistics(classes, form="flow", ts=ts, seed=7)
    assert sorted(set(loaded)) == [1, 3]
    for n, index, a, b, sigma, seed in seen:
        c = int(index[0]) >> 20
        assert n == sizes[c] and torch.equal(index, (c << 20) + torch.arange(n)) and seed == 7
        assert (a, b, sigma) in [A.level_scalars("flow", t) for t in ts]
    assert len(seen) == 10
    seen.clear()
    parts = [A.get_statistics(classes, form="flow", ts=ts, seed=7, rank=r, world=2) for r in (0, 1)]
    assert sorted((int(i[0]) >> 20) for _, i, *_ in seen) == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert parts[0][200]["classes"] == [0, 2, 4] and parts[1][200]["classes"] == [1, 3]
    merged = A.merge_statistics(parts)
    for t in ts:
        w, m = whole[t], merged[t]
        assert np.array_equal(w["hist_x0"], m["hist_x0"]) and np.array_equal(w["hist_xx"], m["hist_xx"])
        assert w["classes"] == m["classes"] == [0, 1, 2, 3, 4] and w["x0_counts"] == m["x0_counts"] and w["xx_counts"] == m["xx_counts"]
        assert w["total_count"] == m["total_count"] == sum(sizes) == w["hist_x0"].sum() == w["hist_xx"].sum()
