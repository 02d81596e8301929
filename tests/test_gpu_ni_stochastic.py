"""GPU tests of the stochastic CIFAR10 step (natinf_step_f64hist_noise, include/natinf.h): matrices whose noise matrix B has
columns beyond the initial noise (SDE Euler-Maruyama, DDIM-eta).  The fused step regenerates eps_j (j >= 1) from
Philox(seed, global image index, column j) in registers; natinf_randn_philox_col_f32 returns the same normals, so the CPU
restatement fed those columns is reproduced bit for bit."""
import re
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from naturaldiffusion_amd import coeffgen as G
from naturaldiffusion_amd.coeff import load_coeff_npz
from oracle import ni_oracle as O
from oracle import philox_oracle as P

SEED = 888
SHAPE = (3, 32, 32)
EPI = 3 * 32 * 32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def gpu_columns(indices, n_cols, dev, epi=EPI):
    """eps_0 .. eps_{n_cols-1} of the given global indices as the fused step injects them (CPU tensors [n, epi]; eps_0 is
    the initial noise generate_sharded draws)"""
    from naturaldiffusion_amd.CIFAR10NaturalInference import philox_noise
    return [philox_noise(indices, (epi,), SEED, dev, column=j).cpu() for j in range(n_cols)]


def ni_stochastic(model, eps, C, B, node, stds=None):
    """CPU restatement of the stochastic CIFAR10 loop (tests/test_ni_stochastic_host.py): CIFAR10-form x0 and signal sum,
    Validate-form noise sum (src/ValidateNaturalInference.py:198-204,349-366)."""
    x, hist, xs = eps[0], [], [eps[0]]
    for k in range(node.shape[0] - 1):
        hist.append(O.cifar_data_fn(model, x, node[k, 0], node[k, 1], node[k, 2], None if stds is None else float(stds[k])))
        m = min(k + 2, B.shape[1])
        x = O.cifar_weighted_sum(C[k], hist) + O.validate_weighted_sum(B[k, :m], eps[:m])
        xs.append(x)
    return xs


def column_noise_oracle(indices, epi, column):
    idx = np.asarray(indices, dtype=np.uint64)
    q = np.arange(epi // 4, dtype=np.uint64)
    c = np.zeros((len(idx), len(q), 4), dtype=np.uint32)
    c[..., 0] = (idx & np.uint64(0xFFFFFFFF))[:, None]
    c[..., 1] = (idx >> np.uint64(32))[:, None]
    c[..., 2] = q[None, :].astype(np.uint32)
    c[..., 3] = np.uint32(column)
    k = np.zeros(c.shape[:-1] + (2,), dtype=np.uint32)
    k[..., 0] = np.uint32(SEED)
    r = P.philox4x32_10(c, k)
    u = ((r >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    out = np.empty(c.shape[:-1] + (4,), dtype=np.float32)
    for h in range(2):
        rad = np.sqrt(np.float32(-2.0) * np.log(u[..., 2 * h]))
        th = np.float32(6.28318530717958647692) * u[..., 2 * h + 1]
        out[..., 2 * h] = rad * np.cos(th)
        out[..., 2 * h + 1] = rad * np.sin(th)
    return out.reshape(len(idx), epi)


# ------------------------------------------------------------------------------ 1. column noise
def test_column_noise(dev):
    from naturaldiffusion_amd.CIFAR10NaturalInference import philox_noise
    idx = [0, 1, 7, 4999, 2 ** 33 + 5]
    base = philox_noise(idx, SHAPE, SEED, dev).cpu()
    col0 = philox_noise(idx, SHAPE, SEED, dev, column=0).cpu()
    assert base.numpy().tobytes() == col0.numpy().tobytes()
    cols = [col0.reshape(len(idx), -1).numpy()]
    for j in (1, 2, 3):
        got = philox_noise(idx, SHAPE, SEED, dev, column=j).cpu().reshape(len(idx), -1).numpy()
        want = column_noise_oracle(idx, EPI, j)
        assert np.abs(got - want).max() < 2e-5                       # integer stream exact; logf / sincosf differ by ulps
        cols.append(got)
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(cols[a], cols[b])
    big = philox_noise(range(256), SHAPE, SEED, dev, column=5).cpu().numpy()
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1.0) < 0.01


# ------------------------------------------------------------------------------ 2. bit-exact trajectories
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("n", [18, 24])
def test_sde_euler_trajectory_bit_exact(dev, repo_root, n, dense):
    """natural_inference on the shipped SDE Euler matrix: every x_k == the CPU restatement fed the kernel's own column noises.
    (Before the fused step the CIFAR10 path read B[k, 0] only and was O(1) off.)"""
    from naturaldiffusion_amd.CIFAR10NaturalInference import natural_inference
    path = repo_root / f"results/euler_heun/sde_euler_{n:03d}.npz"
    C, B, node = load_coeff_npz(path)
    first = 40
    idx = list(range(first, first + 4))
    eps = [c.view(4, *SHAPE) for c in gpu_columns(idx, n + 1, dev)]
    stds = [float(O.vp_std_f32(node[k, 0])) for k in range(n)]
    xs = natural_inference(O.analytic_vp_model(), eps[0].to(dev), path, dense=dense, return_all=True, stds=stds, seed=SEED,
                           first_index=first)
    ref = ni_stochastic(O.analytic_vp_model(), eps, C, B, node, stds)
    assert len(xs) == len(ref) == n + 1
    for k, (x, r) in enumerate(zip(xs, ref)):
        assert np.array_equal(x.cpu().numpy(), r.numpy()), f"x_{k} differs from the restatement"


# ------------------------------------------------------------------------------ 3. classical samplers
@pytest.mark.parametrize("n", [18, 24])
def test_sde_euler_matches_euler_maruyama(dev, repo_root, n):
    from naturaldiffusion_amd.CIFAR10NaturalInference import natural_inference
    path = repo_root / f"results/euler_heun/sde_euler_{n:03d}.npz"
    C, B, node = load_coeff_npz(path)
    idx = list(range(4))
    eps = [c.view(4, *SHAPE) for c in gpu_columns(idx, n + 1, dev)]
    model = O.analytic_vp_model()
    out = natural_inference(model, eps[0].to(dev), path, seed=SEED).cpu().to(torch.float64)
    ts, x = node[:, 0], eps[0].to(torch.float64)
    for i in range(n):
        dt = ts[i + 1] - ts[i]
        beta = 0.1 + ts[i] * (20.0 - 0.1)
        lab = torch.ones(4, dtype=torch.float32) * ts[i] * 999
        score = -model(x.to(torch.float32), lab).to(torch.float64) / float(O.vp_std_f32(ts[i]))
        x = x + (-0.5 * beta * x - beta * score) * dt + np.sqrt(beta) * np.sqrt(abs(dt)) * eps[i + 1].to(torch.float64)
    assert float((out - x).abs().max()) <= 2e-5


def test_ddim_eta1_matches_the_ancestral_loop(dev, tmp_path):
    from naturaldiffusion_amd.CIFAR10NaturalInference import natural_inference
    ts = G.quadratic_time_grid(15)
    C, B, node = G.ddim_vp_continuous(ts, eta=1.0)
    path = tmp_path / "ddim_eta1.npz"
    G.save_coeff_matrix(path, C, B, node)
    eps = [c.view(4, *SHAPE) for c in gpu_columns(range(4), 16, dev)]
    model = O.analytic_vp_model()
    out = natural_inference(model, eps[0].to(dev), path, seed=SEED).cpu().to(torch.float64)
    al, sg = G.vp_alpha_sigma(ts)
    x = eps[0].to(torch.float64)
    for i in range(15):
        lab = torch.ones(4, dtype=torch.float32) * ts[i] * 999
        score = -model(x.to(torch.float32), lab).to(torch.float64) / float(O.vp_std_f32(ts[i]))
        x0 = (x + sg[i] ** 2 * score) / al[i]
        c = (sg[i + 1] / sg[i]) * np.sqrt(1.0 - al[i] ** 2 / al[i + 1] ** 2)
        x = al[i + 1] * x0 + np.sqrt(sg[i + 1] ** 2 - c ** 2) * (x - al[i] * x0) / sg[i] + c * eps[i + 1].to(torch.float64)
    assert float((out - x).abs().max()) <= 2e-5


# ------------------------------------------------------------------------------ 4. column-0 rows through the new entry
def test_column0_rows_through_the_new_entry_are_unchanged(dev, repo_root):
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    from naturaldiffusion_amd.sampler import CifarNI
    C, B, node = load_coeff_npz(repo_root / "weights/step_15_weight_173.npz")
    E = 8 * EPI
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(E, generator=g).to(dev)
    outs = [torch.randn(E, generator=g).to(dev) for _ in range(15)]
    old = CifarNI(C, B, node, E, device=dev)
    new = CifarNI(C, B, node, E, device=dev)
    val_b = torch.tensor([np.float32(B[k, 0]) for k in range(15)], dtype=torch.float32, device=dev)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    xa, xb = noise, noise
    for k in range(15):
        xa = old.step(k, xa, outs[k], noise).clone()
        idx, val, n = new.rows.ptrs(k)
        xn = torch.empty(E, dtype=torch.float32, device=dev)
        rc = lib.natinf_step_f64hist_noise(ptr(xb), ptr(outs[k]), ptr(noise), ptr(new.hist), ptr(xn), idx, val, n,
                                           new.rows.rows[k].diag, ptr(zero), val_b.data_ptr() + 4 * k, 1, k, float(node[k, 1]),
                                           float(node[k, 2]), new.std[k], SEED, None, 0, 1, EPI, E, stream_ptr())
        assert rc == 0
        xb = xn
        assert xa.cpu().numpy().tobytes() == xb.cpu().numpy().tobytes(), f"step {k}"
    assert torch.equal(old.hist.cpu(), new.hist.cpu())


# ------------------------------------------------------------------------------ 5. long history
def test_long_dense_history(dev):
    """120 steps, random dense C and B with zero entries inside rows: the C loop runs past its unroll, the noise loop over 121 columns."""
    from naturaldiffusion_amd.sampler import CifarNI
    rs = np.random.RandomState(9)
    N, n_img, epi = 120, 4, 1024
    E = n_img * epi
    C = np.tril(rs.randn(N, N) * 0.02)                                  # (small enough that 120 steps stay finite)
    Bm = np.zeros((N, N + 1))
    for k in range(N):
        Bm[k, :k + 2] = rs.randn(k + 2) * 0.1
    C[5, 2] = 0.0; C[17, 17] = 0.0; Bm[9, 3] = 0.0; Bm[50, 0] = 0.0
    node = np.zeros((N + 1, 3))
    node[:, 0] = np.linspace(1.0, 1e-3, N + 1)
    node[:, 1] = rs.rand(N + 1) + 0.5
    node[:, 2] = rs.rand(N + 1) + 0.1
    stds = (rs.rand(N) + 0.5).astype(np.float32).tolist()
    g = torch.Generator().manual_seed(3)
    outs = [torch.randn(E, generator=g) for _ in range(N)]
    idx = [1000 + 3 * i for i in range(n_img)]
    eps = gpu_columns(idx, N + 1, dev, epi=epi)
    eps = [e.reshape(-1) for e in eps]
    index = torch.tensor(idx, dtype=torch.int64, device=dev)
    for dense in (False, True):
        ni = CifarNI(C, Bm, node, E, device=dev, dense=dense, stds=stds, seed=SEED, elems_per_image=epi)
        x, xo, hist = eps[0].to(dev), eps[0], []
        nz = eps[0].to(dev)
        for k in range(N):
            x = ni.step(k, x, outs[k].to(dev), nz, index=index)
            hist.append(O.x0_from_score(xo, O.score_from_model_out(outs[k], torch.tensor(stds[k])), node[k, 1], node[k, 2]))
            xo = O.cifar_weighted_sum(C[k], hist) + O.validate_weighted_sum(Bm[k, :k + 2], eps[:k + 2])
            if k % 40 == 39:
                assert torch.equal(x.cpu(), xo), f"step {k} (dense={dense})"
        assert torch.isfinite(xo).all()


# ------------------------------------------------------------------------------ 6. sharding invariance
def test_sharded_generation_is_invariant(dev, repo_root):
    from naturaldiffusion_amd.CIFAR10NaturalInference import generate_sharded
    w = repo_root / "results/euler_heun/sde_euler_018.npz"
    model = O.analytic_vp_model()
    one, i1 = generate_sharded(model, w, 11, 4, rank=0, world=1)
    parts = [generate_sharded(model, w, 11, 3, rank=r, world=2) for r in range(2)]
    full = torch.empty_like(one)
    for im, ix in parts:
        full[ix] = im
    assert torch.equal(i1, torch.arange(11)) and torch.equal(full, one)
    three, _ = generate_sharded([model, model, model], w, 11, 4, streams=3)
    assert torch.equal(three, one)


# ------------------------------------------------------------------------------ 7. drop-in path
def test_natural_inference_tx_with_a_stochastic_matrix(dev, repo_root):
    from naturaldiffusion_amd.CIFAR10NaturalInference import natural_inference, natural_inference_tx
    from naturaldiffusion_amd.ncsnpp import NCSNppEngine, flatten_state_dict
    from naturaldiffusion_amd.synth import synthetic_state_dict
    w = str(repo_root / "results/euler_heun/sde_euler_018.npz")
    flat = flatten_state_dict(synthetic_state_dict(0))
    kw = dict(weight_path=w, flat_params=flat, sample_count=16, batch_size=8, compute_fid=False, device="cuda:0")
    a = natural_inference_tx(streams=3, **kw)
    b = natural_inference_tx(streams=1, **kw)
    assert a.numpy().tobytes() == b.numpy().tobytes()
    from naturaldiffusion_amd.CIFAR10NaturalInference import to_pixel_from_centered
    eng = NCSNppEngine(flat, max_batch=8, device=dev)
    torch.manual_seed(SEED)
    for ii in range(2):
        noise = torch.randn(8, 3, 32, 32, dtype=torch.float32, device=dev)              # natural_inference_tx's draws, in order
        x = natural_inference(eng, noise, w, seed=SEED, first_index=ii * 8)
        assert torch.equal(to_pixel_from_centered(x), a[ii * 8:(ii + 1) * 8]), f"batch {ii}"


# ------------------------------------------------------------------------------ 8. full size
def test_full_size_matches_restatement(dev, repo_root):
    """B = 512 images (E = 512 * 3072), sde_euler_024, random model outputs: the kernel == the CPU restatement, every element."""
    from naturaldiffusion_amd.sampler import CifarNI
    C, B, node = load_coeff_npz(repo_root / "results/euler_heun/sde_euler_024.npz")
    n, n_img = 24, 512
    E = n_img * EPI
    g = torch.Generator().manual_seed(12)
    outs = [torch.randn(E, generator=g) for _ in range(n)]
    stds = [float(O.vp_std_f32(node[k, 0])) for k in range(n)]
    eps = [e.reshape(-1) for e in gpu_columns(range(n_img), n + 1, dev)]
    ni = CifarNI(C, B, node, E, device=dev, stds=stds, seed=SEED, elems_per_image=EPI)
    x, nz = eps[0].to(dev), eps[0].to(dev)
    xo, hist = eps[0], []
    for k in range(n):
        x = ni.step(k, x, outs[k].to(dev), nz, index=0)
        hist.append(O.x0_from_score(xo, O.score_from_model_out(outs[k], torch.tensor(stds[k])), node[k, 1], node[k, 2]))
        xo = O.cifar_weighted_sum(C[k], hist) + O.validate_weighted_sum(B[k, :k + 2], eps[:k + 2])
    assert torch.equal(x.cpu(), xo)
    assert torch.equal(ni.hist[n - 1].cpu(), hist[-1])


# ------------------------------------------------------------------------------ 9. ISA and refusals
def _kernels(listing):
    """demangled name -> (vgpr spills, sgpr spills, scratch bytes) from the amdhsa.kernels metadata"""
    md = listing[listing.index("amdhsa.kernels:"):]
    rows = []
    for blk in re.split(r"\n  - \.", md)[1:]:
        get = lambda key: re.search(r"\." + key + r":\s*(\S+)", blk).group(1)
        rows.append((get("name"), int(get("vgpr_spill_count")), int(get("sgpr_spill_count")), int(get("private_segment_fixed_size"))))
    names = subprocess.run(["c++filt"] + [r[0] for r in rows], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return {nm: r[1:] for nm, r in zip(names, rows)}


def test_fused_step_does_not_spill(repo_root):
    csrc = repo_root / "naturaldiffusion_amd" / "csrc"
    subprocess.check_call(["make", "-C", str(csrc), "-j4"], stdout=subprocess.DEVNULL)
    ks = _kernels((csrc / "build" / "ni_step-hip-amdgcn-amd-amdhsa-gfx950.s").read_text())
    mine = {nm: v for nm, v in ks.items() if "k_step_noise_f64" in nm}
    assert len(mine) == 1 and all(v == (0, 0, 0) for v in mine.values()), mine


def test_refusals(dev, repo_root):
    from naturaldiffusion_amd._lib import lib, ptr
    from naturaldiffusion_amd.sampler import CifarNI
    C, B, node = load_coeff_npz(repo_root / "results/euler_heun/sde_euler_018.npz")
    with pytest.raises(ValueError):
        CifarNI(C, B, node, 4 * EPI, device=dev)                             # no seed
    with pytest.raises(ValueError):
        CifarNI(C, B, node, 4 * EPI, device=dev, seed=1, fast_f32=True)
    ni = CifarNI(C, B, node, 4 * EPI, device=dev, seed=1)
    t = torch.zeros(4 * EPI, device=dev)
    with pytest.raises(ValueError):
        ni.step(0, t, t, t)                                                  # elems_per_image unknown outside run()
    x = torch.zeros(8, device=dev)
    h = torch.zeros(8, dtype=torch.float64, device=dev)
    ib = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    vb = torch.tensor([0.5, 0.5], dtype=torch.float32, device=dev)
    step = lambda epi, E: lib.natinf_step_f64hist_noise(ptr(x), ptr(x), ptr(x), ptr(h), ptr(x), None, None, 0, 1.0, ptr(ib), ptr(vb), 2,
                                                         0, 1.0, 0.5, 1.0, SEED, None, 0, 1, epi, E, None)
    assert step(4 * 2 ** 32, 4 * 2 ** 32) == -1                               # quad count does not fit counter word 2
    assert step(6, 12) == -1 and step(8, 12) == -1 and step(0, 8) == -1
    assert lib.natinf_randn_philox_col_f32(ptr(x), 1, 4 * 2 ** 32, None, 0, 1, SEED, 1, None) == -1
    assert step(4, 8) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ 10. run() goes through the instance's step
@pytest.mark.parametrize("rel", ["weights/step_5_weight_00", "results/euler_heun/sde_euler_018"])
def test_run_calls_the_instance_step(dev, repo_root, rel):
    """CifarNI.run issues every step through ``self.step``, so a per-instance wrapper (bench.py's event-timed replica) sees all
    of them; a column-0 matrix still gets the four positional arguments only."""
    from naturaldiffusion_amd.sampler import CifarNI
    C, B, node = load_coeff_npz(repo_root / f"{rel}.npz")
    ni = CifarNI(C, B, node, 2 * EPI, device=dev, seed=SEED)
    seen, orig = [], ni.step

    def wrapped(k, *a, **kw):
        seen.append((k, len(a), sorted(kw)))
        return orig(k, *a, **kw)
    ni.step = wrapped
    noise = gpu_columns(range(2), 1, dev)[0].view(2, *SHAPE).to(dev)
    ni.run(O.analytic_vp_model(), noise)
    n = C.shape[0]
    assert [s[0] for s in seen] == list(range(n))
    if ni.stochastic:
        assert all(s[1:] == (3, ["elems_per_image", "index"]) for s in seen)
    else:
        assert all(s[1:] == (3, []) for s in seen)


def test_bench_full_roofline_replica(dev, repo_root):
    """bench.py --full with the event-instrumented replica on (small batch, extras off): it wraps ni.step and must time every step."""
    import json
    import os
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, str(repo_root / "bench.py"), "--gpus", "1", "--batch", "64", "--steps", "1", "--warmup", "1", "--full",
                        "--no-sd3", "--no-validate", "--no-fid50k", "--no-cpu-baseline"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    r = line["roofline_ni_step"]
    assert r["achieved"] > 0 and r["mean_launch_ms"] > 0
