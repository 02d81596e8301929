"""Stochastic Natural Inference matrices on the host (no GPU): which shipped matrices inject noise after a step, the DDIM-eta
generator on the continuous VP grid, and the CPU restatement of the stochastic CIFAR10 loop

    x_{k+1} = fp32(sum_j C[k,j] x0_j) + fp32(sum_j fp32(B[k,j] eps_j))      (src/ValidateNaturalInference.py:349-366)

against the classical fp64 samplers the matrices were unrolled from (Euler-Maruyama, DDIM-eta), with Philox noises keyed like
natinf_randn_philox_col_f32 (counter word 3 = the column of B)."""
import numpy as np
import pytest
import torch

from naturaldiffusion_amd import coeffgen as G
from naturaldiffusion_amd.coeff import is_stochastic, load_coeff_npz
from oracle import ni_oracle as O
from oracle import philox_oracle as P

SEED, N_IMG, EPI = 888, 4, 3 * 32 * 32


def column_noise(indices, elems_per_image, seed, column):
    """float32 [len(indices), elems_per_image]: philox_oracle.randn's layout with counter word 3 = ``column`` (column 0 is randn itself)."""
    if column == 0:
        return P.randn(indices, elems_per_image, seed)[0]
    idx = np.asarray(indices, dtype=np.uint64)
    q = np.arange(elems_per_image // 4, dtype=np.uint64)
    c = np.zeros((len(idx), len(q), 4), dtype=np.uint32)
    c[..., 0] = (idx & np.uint64(0xFFFFFFFF))[:, None]
    c[..., 1] = (idx >> np.uint64(32))[:, None]
    c[..., 2] = q[None, :].astype(np.uint32)
    c[..., 3] = np.uint32(column)
    k = np.zeros(c.shape[:-1] + (2,), dtype=np.uint32)
    k[..., 0] = np.uint32(seed & 0xFFFFFFFF); k[..., 1] = np.uint32((seed >> 32) & 0xFFFFFFFF)
    r = P.philox4x32_10(c, k)
    u = ((r >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    out = np.empty(c.shape[:-1] + (4,), dtype=np.float32)
    for h in range(2):
        rad = np.sqrt(np.float32(-2.0) * np.log(u[..., 2 * h]))
        th = np.float32(6.28318530717958647692) * u[..., 2 * h + 1]
        out[..., 2 * h] = rad * np.cos(th)
        out[..., 2 * h + 1] = rad * np.sin(th)
    return out.reshape(len(idx), elems_per_image)


def noises(n_cols, shape=(N_IMG, 3, 32, 32)):
    return [torch.from_numpy(column_noise(range(shape[0]), EPI, SEED, j)).view(shape) for j in range(n_cols)]


def ni_stochastic(model, eps, C, B, node):
    """CPU restatement of the stochastic CIFAR10 loop: the CIFAR10 form's x0 and signal sum, the Validate form's noise sum."""
    x, hist, xs = eps[0], [], [eps[0]]
    for k in range(node.shape[0] - 1):
        hist.append(O.cifar_data_fn(model, x, node[k, 0], node[k, 1], node[k, 2]))
        m = min(k + 2, B.shape[1])
        x = O.cifar_weighted_sum(C[k], hist) + O.validate_weighted_sum(B[k, :m], eps[:m])
        xs.append(x)
    return xs


def model_eval(model, x64, t):
    """the stand-in network on the fp32 state, its score -out/std in fp64 (models/utils.py:157)"""
    labels = torch.ones(x64.shape[0], dtype=torch.float32) * t * 999
    return -model(x64.to(torch.float32), labels).to(torch.float64) / float(O.vp_std_f32(t))


@pytest.mark.parametrize("rel,want", [("weights/step_5_weight_00", False), ("weights/step_10_weight_42", False),
                                      ("weights/step_15_weight_173", False), ("results/euler_heun/ode_euler_018", False),
                                      ("results/euler_heun/ode_euler_024", False), ("results/dpmsolver/dpmsolver2s_018", False),
                                      ("results/dpmsolver/dpmsolver3s_024", False), ("results/dpmsolverpp/dpmsolverpp2s_018", False),
                                      ("results/dpmsolverpp/dpmsolverpp3s_024", False), ("results/euler_heun/sde_euler_018", True),
                                      ("results/euler_heun/sde_euler_024", True)])
def test_is_stochastic_on_shipped_matrices(repo_root, rel, want):
    C, B, node = load_coeff_npz(repo_root / f"{rel}.npz")
    assert is_stochastic(B) is want


def test_is_stochastic_edges():
    assert not is_stochastic(np.zeros((3, 4)))
    assert not is_stochastic(np.array([[0.5], [0.25]]))
    B = np.zeros((3, 4)); B[:, 0] = 1.0
    assert not is_stochastic(B)
    B[2, 3] = 1e-30
    assert is_stochastic(B)
    assert is_stochastic(G.vp_euler(6, stochastic=True)[1]) and not is_stochastic(G.vp_euler(6)[1])


def test_column_noise_oracle_column_zero_is_randn():
    x = column_noise([0, 5, 2 ** 33 + 1], EPI, SEED, 0)
    y = column_noise([0, 5, 2 ** 33 + 1], EPI, SEED, 1)
    assert np.array_equal(x, P.randn([0, 5, 2 ** 33 + 1], EPI, SEED)[0])
    assert not np.array_equal(x, y) and abs(y.mean()) < 0.05 and abs(y.std() - 1) < 0.05


def test_ddim_eta_zero_is_the_closed_form():
    ts = G.quadratic_time_grid(15)
    C0, B0, n0 = G.ddim_vp_continuous(ts)
    C1, B1, n1 = G.ddim_vp_continuous(ts, eta=0)
    assert np.array_equal(C0, C1) and np.array_equal(B0, B1) and np.array_equal(n0, n1)
    C2, B2, n2 = G.ddim_vp_continuous(ts, eta=0.5)
    assert C2.shape == C0.shape and B2.shape == (15, 16) and np.array_equal(n2, n0)
    assert is_stochastic(B2) and not is_stochastic(B0)
    assert all(np.count_nonzero(B2[k, k + 2:]) == 0 and B2[k, k + 1] != 0 for k in range(15))   # eps_{k+1} enters at step k


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_ddim_eta_matrix_matches_the_classical_loop(eta):
    """the NI restatement of coeffgen.ddim_vp_continuous(ts, eta) == the classical fp64 DDIM-eta loop (15-step quadratic grid,
    4 images, the stand-in model, Philox noises) within 1e-6."""
    ts = G.quadratic_time_grid(15)
    C, B, node = G.ddim_vp_continuous(ts, eta=eta)
    model = O.analytic_vp_model()
    eps = noises(16)
    ni = ni_stochastic(model, eps, C, B, node)[-1]
    al, sg = G.vp_alpha_sigma(ts)
    x = eps[0].to(torch.float64)
    for i in range(15):
        score = model_eval(model, x, ts[i])
        x0 = (x + sg[i] ** 2 * score) / al[i]
        eps_hat = (x - al[i] * x0) / sg[i]
        c = eta * (sg[i + 1] / sg[i]) * np.sqrt(1.0 - al[i] ** 2 / al[i + 1] ** 2)
        x = al[i + 1] * x0 + np.sqrt(sg[i + 1] ** 2 - c ** 2) * eps_hat + c * eps[i + 1].to(torch.float64)
    err = float((ni.to(torch.float64) - x).abs().max())
    assert err <= 1e-6, err


@pytest.mark.parametrize("n", [18, 24])
def test_sde_euler_matrix_matches_euler_maruyama(repo_root, n):
    """the shipped results/euler_heun/sde_euler_0NN.npz through the NI restatement == fp64 Euler-Maruyama on the reverse VP SDE
    (src/AnalyzeEulerHeun.py:125-200) within 1e-6; column 0 alone (what the CIFAR10 path used to read) is O(1) away."""
    C, B, node = load_coeff_npz(repo_root / f"results/euler_heun/sde_euler_{n:03d}.npz")
    model = O.analytic_vp_model()
    eps = noises(n + 1)
    ni = ni_stochastic(model, eps, C, B, node)[-1]
    ts = node[:, 0]
    x = eps[0].to(torch.float64)
    for i in range(n):
        dt = ts[i + 1] - ts[i]
        beta = 0.1 + ts[i] * (20.0 - 0.1)
        f, g = -0.5 * beta, np.sqrt(beta)
        x = x + (f * x - g ** 2 * model_eval(model, x, ts[i])) * dt + g * np.sqrt(abs(dt)) * eps[i + 1].to(torch.float64)
    err = float((ni.to(torch.float64) - x).abs().max())
    assert err <= 1e-6, err
    col0 = O.cifar_ni_trajectory(model, eps[0], C, B, node)[-1]
    assert float((col0.to(torch.float64) - x).abs().max()) > 0.1
