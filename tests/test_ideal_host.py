"""Host side of the ideal denoiser (include/natinf_ideal.h; naturaldiffusion_amd/ideal.py): the fp64 oracle's own limits, the level scalars and the eps
form's round trip through the step's x0 formula, the label -> level mapping, every refusal of the C entries with no device present, the workspace query and
the Python layer's shape and dtype errors.  No GPU."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import ideal_oracle as O
from naturaldiffusion_amd import _lib, coeffgen
from naturaldiffusion_amd import ideal as I

EINVAL = -1
L = _lib.lib
PTR = 0x1000            # 256-byte aligned, non-null, never dereferenced: every call below must be refused before anything is configured or launched


# ---- the oracle's limits ----

def _set(n, d, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, d)).astype(np.float64)


def test_oracle_c_zero_is_the_column_mean():
    f, u = _set(37, 64, 1), _set(5, 64, 2)
    r = O.posterior_mean(u, 0.0, f)
    assert np.allclose(r["x0"], f.mean(0)[None].repeat(5, 0), rtol=1e-14, atol=0) and np.allclose(r["pmax"], 1 / 37, rtol=1e-14)
    assert np.allclose(r["lse"], np.log(37.0), rtol=1e-14)
    r = O.posterior_mean(f[:5], 0.0, f, self_offset=0)                   # the left-out row is out of the mean as well: the select, not 0 * inf
    want = np.stack([np.delete(f, i, 0).mean(0) for i in range(5)])
    assert np.isfinite(r["x0"]).all() and np.allclose(r["x0"], want, rtol=1e-13) and (r["p"][np.arange(5), np.arange(5)] == 0).all()


def test_oracle_huge_c_is_the_nearest_row():
    f, u = _set(37, 64, 3), _set(6, 64, 4)
    r = O.posterior_mean(u, 1e6, f)
    near = np.argmin(O.dist2(u, f), 1)
    assert np.array_equal(r["nearest"], near) and np.array_equal(r["x0"], f[near]) and (r["pmax"] == 1.0).all()
    r0 = O.posterior_mean(f[10:16], 1e6, f, self_offset=10)              # its own row left out: the second nearest
    assert not (r0["nearest"] == 10 + np.arange(6)).any() and np.array_equal(r0["x0"], f[r0["nearest"]])


def test_oracle_duplicate_rows_give_that_row():
    f = _set(20, 64, 5)
    f[13] = f[4]
    u = f[[4]] + 1.0
    r = O.posterior_mean(u, 1.0, f)                                      # the two logits are -64, every other one below -10^4
    # two equal weights of one half, the lower index reported.  lse = m + log 2 is rounded at ulp(m) = 2^-47, so p = exp(z - lse) is one half to within
    # that (relative); the device's w = fp32(p) is 0.5 exactly
    assert r["nearest"][0] == 4 and np.allclose(r["x0"][0], f[4], rtol=2.0 ** -45, atol=0) and abs(r["pmax"][0] - 0.5) <= 2.0 ** -46
    assert r["p"][0, 4] == r["p"][0, 13] and np.float32(r["p"][0, 4]) == np.float32(0.5) and r["p"][0].sum() - 2 * r["p"][0, 4] == 0.0


# ---- levels ----

def test_level_scalars_and_the_eps_form_round_trip():
    rng = np.random.default_rng(7)
    f = (rng.integers(0, 256, (50, 64)) + 0.5) / 255 * 2 - 1
    ts = np.array([1.0, 0.5, 0.1, 1e-3])
    alpha, sigma = coeffgen.vp_alpha_sigma(ts)
    x = (alpha[:, None] * f[:4] + sigma[:, None] * rng.standard_normal((4, 64))).astype(np.float32)
    u, c = I.level_scalars(torch.from_numpy(x), alpha, sigma)
    assert u.dtype == torch.float32 and isinstance(c, np.ndarray) and c.dtype == np.float64
    assert np.array_equal(u.numpy(), (x.astype(np.float64) / alpha[:, None]).astype(np.float32)) and np.array_equal(c, alpha ** 2 / (2 * sigma ** 2))
    # -c |u - f|^2 is the log-likelihood -|x - alpha f|^2 / (2 sigma^2) of x_t = alpha f + sigma eps
    loglik = np.stack([-((x[i].astype(np.float64) - alpha[i] * f) ** 2).sum(1) / (2 * sigma[i] ** 2) for i in range(4)])
    assert np.allclose(-c[:, None] * O.dist2(u.numpy(), f), loglik, rtol=1e-5)
    r = O.posterior_mean(u.numpy(), c, f, x=x, alpha=alpha, sigma=sigma)
    out32 = r["out"].astype(np.float32)
    for i in range(4):                                                   # natinf_step_f64hist's formula with std = sigma gives the posterior mean back
        back = O.step_x0(out32[i], x[i], alpha[i], sigma[i], std=sigma[i])
        assert np.abs(back - r["x0"][i]).max() <= 2.0 ** -23 * np.abs(out32[i]).max() * sigma[i] / alpha[i] + 1e-15, i
    # scalars broadcast; device-less tensors of levels take the tensor path
    u1, c1 = I.level_scalars(torch.from_numpy(x), float(alpha[1]), float(sigma[1]))
    assert c1.shape == (4,) and (c1 == c[1]).all() and np.array_equal(u1[1].numpy(), u[1].numpy())
    u2, c2 = I.level_scalars(torch.from_numpy(x), torch.from_numpy(alpha), torch.from_numpy(sigma))
    assert isinstance(c2, torch.Tensor) and c2.dtype == torch.float64 and np.array_equal(c2.numpy(), c) and torch.equal(u2, u)
    for bad in ((0.5, 0.0), (0.5, -1.0), (0.0, 0.5), (np.nan, 0.5), (0.5, np.inf)):
        with pytest.raises(ValueError, match="ideal"):
            I.level_scalars(torch.from_numpy(x), *bad)
    with pytest.raises(ValueError, match="fp32"):
        I.level_scalars(torch.from_numpy(x).double(), 0.5, 0.5)


def test_label_to_level_mapping_is_coeffgens():
    ts = coeffgen.quadratic_time_grid(10)
    labels = np.array([float(np.float32(t) * np.float32(999)) for t in ts], np.float32)        # CifarNI's labels
    alpha, sigma = I.levels_of_labels(torch.from_numpy(labels))
    want_a, want_s = coeffgen.vp_alpha_sigma(labels.astype(np.float64) / 999.0)
    assert alpha.dtype == np.float64 and np.array_equal(alpha, want_a) and np.array_equal(sigma, want_s)
    node_a, node_s = coeffgen.vp_alpha_sigma(ts)                         # the job's own nodes, up to the label's fp32 rounding
    assert np.allclose(alpha, node_a, rtol=1e-5) and np.allclose(sigma, node_s, rtol=1e-5)
    assert np.allclose(alpha ** 2 + sigma ** 2, 1.0, rtol=1e-14)


# ---- the C entries with no device ----

def _pm(rows=PTR, c=PTR, n_rows=4, cp=PTR, cn=PTR, ct=PTR, n_cols=8, d=64, self_offset=-1, x=None, alpha=None, sigma=None, x0=PTR, lse=None, pmax=None,
        nearest=None, out=None, ws=PTR, ws_bytes=1 << 40):
    return L.natinf_ideal_posterior_mean(rows, c, n_rows, cp, cn, ct, n_cols, d, self_offset, x, alpha, sigma, x0, lse, pmax, nearest, out, ws, ws_bytes, None)


def _dw(rows=PTR, c=PTR, n_rows=4, cp=PTR, cn=PTR, n_cols=8, d=64, self_offset=-1, w=PTR, planes=None, ws=PTR, ws_bytes=1 << 40):
    return L.natinf_ideal_debug_weights(rows, c, n_rows, cp, cn, n_cols, d, self_offset, w, planes, ws, ws_bytes, None)


def test_argument_errors_are_einval_without_a_device():
    for fn in (_pm, _dw):
        for d in (0, 32, 96, -64, 4096 + 64, 65536):
            assert fn(d=d) == EINVAL, d
        for n in (0, -1, (1 << 20) + 1):
            assert fn(n_rows=n) == EINVAL and fn(n_cols=n) == EINVAL, n
        for so in (-2, 5, 8, 1 << 40):                                   # the left-out column must exist for every row
            assert fn(self_offset=so) == EINVAL, so
        assert fn(n_rows=1, n_cols=1, self_offset=0) == EINVAL           # nothing would be left
        for name in ("rows", "c", "cp", "cn", "ws"):
            assert fn(**{name: None}) == EINVAL, name
        assert fn(rows=PTR + 8) == EINVAL and fn(cp=PTR + 8) == EINVAL and fn(c=PTR + 4) == EINVAL and fn(cn=PTR + 4) == EINVAL
        assert fn(ws=PTR + 16) == EINVAL and fn(ws=PTR + 128) == EINVAL
        need = L.natinf_ideal_workspace_bytes(4, 8, 64)
        assert need > 0 and fn(ws_bytes=need - 1) == EINVAL and fn(ws_bytes=0) == EINVAL and fn(ws_bytes=-1) == EINVAL
    assert _pm(ct=None) == EINVAL and _pm(ct=PTR + 8) == EINVAL and _pm(x0=None) == EINVAL and _pm(x0=PTR + 2) == EINVAL
    assert _pm(lse=PTR + 4) == EINVAL and _pm(pmax=PTR + 4) == EINVAL and _pm(nearest=PTR + 2) == EINVAL
    # x, alpha, sigma and out: all four or none
    full = dict(x=PTR, alpha=PTR, sigma=PTR, out=PTR)
    for name in full:
        assert _pm(**{name: PTR}) == EINVAL, name
        assert _pm(**{k: v for k, v in full.items() if k != name}) == EINVAL, name
    assert _pm(**{**full, "x": PTR + 2}) == EINVAL and _pm(**{**full, "out": PTR + 2}) == EINVAL
    assert _pm(**{**full, "alpha": PTR + 4}) == EINVAL and _pm(**{**full, "sigma": PTR + 4}) == EINVAL
    assert _dw(w=None) == EINVAL and _dw(w=PTR + 2) == EINVAL and _dw(planes=PTR + 8) == EINVAL
    assert _dw(n_rows=1025, n_cols=1024) == EINVAL                       # the test hook's 2^20 entries
    for bad in (dict(planes=None), dict(planes=PTR + 8), dict(out=None), dict(out=PTR + 8), dict(n=0), dict(n=(1 << 20) + 1), dict(d=96), dict(d=8192)):
        kw = {**dict(planes=PTR, n=8, d=64, out=PTR), **bad}
        assert L.natinf_ideal_tplanes(kw["planes"], kw["n"], kw["d"], kw["out"], None) == EINVAL, bad


def test_workspace_bytes_is_monotone_and_negative_outside_the_limits():
    ns = [1, 2, 63, 64, 65, 255, 256, 257, 300, 1000, 50000, 1 << 20]
    cols = [1, 8, 63, 64, 65, 2047, 2048, 2049, 2112, 2113, 5000, 50000, 1 << 20]
    ds = [64, 128, 192, 2048, 3072, 4096]
    b = np.array([[[L.natinf_ideal_workspace_bytes(n, c, d) for d in ds] for c in cols] for n in ns], dtype=np.int64)
    assert (b > 0).all() and all((np.diff(b, axis=a) >= 0).all() for a in range(3))
    assert b[ns.index(256)].tolist() == b[ns.index(1 << 20)].tolist()    # a chunk of rows at a time: no term grows beyond NATINF_IDEAL_CHUNK_ROWS rows
    assert L.natinf_ideal_workspace_bytes(256, 50000, 3072) < 1 << 29    # 102 MB of distances, 77 MB of weight planes, 157 MB of partial sums
    for d in (0, 32, 96, -64, 4096 + 64):
        assert L.natinf_ideal_workspace_bytes(4, 8, d) == EINVAL, d
    for n in (0, -1, (1 << 20) + 1):
        assert L.natinf_ideal_workspace_bytes(n, 8, 64) == EINVAL and L.natinf_ideal_workspace_bytes(4, n, 64) == EINVAL, n


def test_the_python_constants_are_the_headers(repo_root):
    import re
    text = (repo_root / "include" / "natinf_ideal.h").read_text()
    get = lambda name: int(re.search(r"#define " + name + r" (\d+)", text).group(1))
    assert get("NATINF_IDEAL_K_RANGE") == I.K_RANGE and get("NATINF_IDEAL_CHUNK_ROWS") == I.CHUNK_ROWS
    assert I.K_RANGE % 64 == 0 and I.CHUNK_ROWS % 64 == 0 and I.padded_cols(1) == 64 and I.padded_cols(64) == 64 and I.padded_cols(65) == 128


# ---- the Python layer's refusals (all raised before the library is touched) ----

class _FakeTrain(I.TrainingSet):
    def __init__(self, n, d):
        self.n, self.d, self.device = n, d, torch.device("cpu")


def test_python_shape_and_dtype_errors():
    tr = _FakeTrain(10, 64)
    ok = torch.zeros(3, 64)
    for bad in (torch.zeros(3, 64, dtype=torch.float64), torch.zeros(3, 128), torch.zeros(64), torch.zeros(3, 64, dtype=torch.int32)):
        with pytest.raises(ValueError, match="ideal: rows"):
            I.posterior_mean(bad, 1.0, tr)
    with pytest.raises(ValueError, match="TrainingSet"):
        I.posterior_mean(ok, 1.0, torch.zeros(10, 64))
    for c in (-1.0, np.nan, np.inf, [1.0, 2.0], [1.0, -0.0, -1e-300], torch.tensor([1.0, np.nan, 1.0])):
        with pytest.raises(ValueError, match="ideal: c"):
            I.posterior_mean(ok, c, tr)
    for kw in (dict(x=ok), dict(alpha=1.0), dict(x=ok, alpha=1.0), dict(alpha=1.0, sigma=1.0)):
        with pytest.raises(ValueError, match="come together"):
            I.posterior_mean(ok, 1.0, tr, **kw)
    with pytest.raises(ValueError, match="ideal: x"):
        I.posterior_mean(ok, 1.0, tr, x=torch.zeros(3, 32), alpha=1.0, sigma=1.0)
    with pytest.raises(ValueError, match="differ"):
        I.posterior_mean(ok, 1.0, tr, x=torch.zeros(2, 64), alpha=1.0, sigma=1.0)
    for sg in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="ideal: sigma"):
            I.posterior_mean(ok, 1.0, tr, x=ok, alpha=1.0, sigma=sg)
    for so in (-2, 8, 10):
        with pytest.raises(ValueError, match="self_offset"):
            I.posterior_mean(ok, 1.0, tr, self_offset=so)
    with pytest.raises(ValueError, match="too small"):
        I.posterior_mean(ok[:1], 1.0, _FakeTrain(1, 64), self_offset=0)
    for bad in (torch.zeros(4, 96), torch.zeros(4, 32), torch.zeros(4, 8192), torch.zeros(4, 64, dtype=torch.float64), torch.zeros(64)):
        with pytest.raises(ValueError, match="ideal"):
            I.TrainingSet(bad, device="cpu")
    for bad in (torch.zeros(2, 32, 32, 3), torch.zeros(2, 3, 32, 32, dtype=torch.uint8), torch.zeros(2, 16, 16, 3, dtype=torch.uint8), torch.zeros(2, 3072)):
        with pytest.raises(ValueError, match="train_images"):
            I.train_images_to_feats(bad)
    u8 = torch.arange(2 * 32 * 32 * 3, dtype=torch.int64).remainder(256).to(torch.uint8).reshape(2, 32, 32, 3)
    from naturaldiffusion_amd.CIFAR10NaturalInference import u8_to_centered
    assert torch.equal(I.train_images_to_feats(u8), u8_to_centered(u8.permute(0, 3, 1, 2)).reshape(2, -1))


def test_module_imports_without_the_library(repo_root, tmp_path):
    code = ("import os, sys; os.environ['NATINF_LIB'] = sys.argv[2]; sys.path.insert(0, sys.argv[1])\n"
            "import torch\n"
            "from naturaldiffusion_amd import ideal as I\n"
            "assert 'naturaldiffusion_amd._lib' not in sys.modules\n"
            "u, c = I.level_scalars(torch.ones(2, 64), 0.5, 0.25)\n"
            "print(float(u[0, 0]), float(c[0]))\n")
    p = subprocess.run([sys.executable, "-c", code, str(repo_root), str(tmp_path / "absent.so")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.split() == ["2.0", "2.0"]
