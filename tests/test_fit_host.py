"""Host side of the coefficient fitter (include/natinf_fit.h; naturaldiffusion_amd/fit.py): every refusal of natinf_fit_gram_f64 with no device present,
the row solver on synthetic Gram matrices (recovery, the sum constraint, the support, KKT, the residual identity, ridge), fit_matrix's refusals before
anything needs a GPU, and the node match of the shipped 5-step matrix against a DDIM teacher on the 20-step quadratic grid.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import fit_oracle as O
from naturaldiffusion_amd import _lib, coeffgen
from naturaldiffusion_amd import fit as F
from naturaldiffusion_amd.coeff import load_coeff_npz

EINVAL = -1
L = _lib.lib
PTR = 0x1000            # 16-byte aligned, non-null, never dereferenced: every call below must be refused before anything is configured or launched


def _call(hist=PTR, stride=8 * 3072, rows=(0, 1, 2), n_rows=None, noise=PTR, target=PTR, n_images=8, epi=3072, gram=PTR):
    arr = (ctypes.c_int32 * max(len(rows), 1))(*rows)
    return L.natinf_fit_gram_f64(hist, stride, arr, len(rows) if n_rows is None else n_rows, noise, target, n_images, epi, gram, None)


@pytest.mark.parametrize("kw", [
    dict(rows=(), n_rows=0), dict(rows=tuple(range(31))),                                   # 1 <= n_rows <= 30
    dict(rows=(0, 2, 2)), dict(rows=(0, 3, 1)), dict(rows=(-1, 0, 1)),                      # strictly ascending, non-negative
    dict(epi=0), dict(epi=3070), dict(epi=2), dict(epi=(1 << 24) + 4, stride=8 * ((1 << 24) + 4)),
    dict(n_images=0), dict(n_images=(1 << 20) + 1, epi=4, stride=4 * ((1 << 20) + 1)),
    dict(stride=8 * 3072 - 4), dict(stride=8 * 3072 + 1),                                   # the slab holds every image; 16-byte rows
    dict(hist=PTR + 8), dict(noise=PTR + 4), dict(target=PTR + 8), dict(gram=PTR + 8),      # 16-byte alignment
    dict(hist=0), dict(noise=0), dict(target=0), dict(gram=0),
], ids=lambda kw: ",".join(f"{k}={v if not isinstance(v, tuple) or len(v) < 5 else len(v)}" for k, v in kw.items()))
def test_gram_entry_refuses_before_any_launch(kw):
    assert _call(**kw) == EINVAL


def test_gram_entry_refuses_null_rows():
    assert L.natinf_fit_gram_f64(PTR, 8 * 3072, None, 3, PTR, PTR, 8, 3072, PTR, None) == EINVAL


# ---- solve_row on a synthetic Gram matrix ----

@pytest.fixture(scope="module")
def synth():
    """6 random vectors of 512 values, a noise vector, c* with a known sum, and the target sum_j c*_j v_j + b0 noise"""
    rng = np.random.default_rng(11)
    V, noise = rng.standard_normal((6, 512)), rng.standard_normal(512)
    c, b0 = rng.standard_normal(6), 0.37
    target = c @ V + b0 * noise
    stack = np.vstack([V, noise, target])
    return dict(V=V, noise=noise, c=c, b0=b0, target=target, G=O.gram(stack)[0])


def test_solve_row_recovers_the_coefficients(synth):
    for row_sum in (float(np.sum(synth["c"])), None):
        c = F.solve_row(synth["G"], row_sum, b0=synth["b0"])
        assert np.abs(c - synth["c"]).max() <= 1e-9, row_sum
    assert np.abs(O.solve_row(synth["G"], float(np.sum(synth["c"])), b0=synth["b0"]) - synth["c"]).max() <= 1e-9      # the oracle's other route


@pytest.mark.parametrize("support", [None, [1, 4], [0, 2, 3, 5], [5]])
@pytest.mark.parametrize("row_sum", [0.9, -3.25, 1e-3])
def test_sum_constraint_support_and_kkt(synth, support, row_sum):
    G, b0 = synth["G"], synth["b0"]
    c = F.solve_row(G, row_sum, b0=b0, support=support)
    sup = list(range(6)) if support is None else support
    n = len(sup)
    assert abs(float(np.sum(c)) - row_sum) <= 4 * n * 2.0 ** -53 * np.abs(c).sum()
    assert all(c[j] == 0.0 for j in range(6) if j not in sup)
    grad = (G[:6, :6] @ c - (G[:6, 7] - b0 * G[:6, 6]))[sup]                 # constant over the supported columns: the multiplier of the sum
    assert np.abs(grad - grad.mean()).max() <= 1e-9 * np.linalg.norm(grad)
    if n > 1:
        assert np.abs(c - O.solve_row(G, row_sum, b0=b0, support=support)).max() <= 1e-9 * np.abs(c).max()


def test_unconstrained_gradient_vanishes(synth):
    G = synth["G"].copy()
    rng = np.random.default_rng(5)
    other = rng.standard_normal(512)                                          # a target outside the span: a true least-squares problem
    G = O.gram(np.vstack([synth["V"], synth["noise"], other]))[0]
    c = F.solve_row(G, None, b0=0.2, support=[0, 1, 3])
    g = G[:6, 7] - 0.2 * G[:6, 6]
    assert np.abs((G[:6, :6] @ c - g)[[0, 1, 3]]).max() <= 1e-9 * np.linalg.norm(g) and c[2] == c[4] == c[5] == 0.0


def test_row_residual_is_the_squared_norm(synth):
    rng = np.random.default_rng(6)
    for _ in range(4):
        c, b0 = rng.standard_normal(6), float(rng.standard_normal())
        direct = float(np.sum((c @ synth["V"] + b0 * synth["noise"] - synth["target"]).astype(np.longdouble) ** 2))
        assert abs(F.row_residual(synth["G"], c, b0) - direct) <= 1e-10 * direct


def test_ridge_does_not_increase_the_coefficients():
    rng = np.random.default_rng(8)
    base = rng.standard_normal(512)
    V = base + 1e-3 * rng.standard_normal((6, 512))                           # nearly parallel vectors, as a history's are
    G = O.gram(np.vstack([V, rng.standard_normal(512), rng.standard_normal(512)]))[0]
    prev = None
    for ridge in (0.0, 1e-8, 1e-4, 1e-1):
        for row_sum in (1.0, None):
            c = F.solve_row(G, row_sum, b0=0.1, ridge=ridge)
            if row_sum is not None:
                assert abs(c.sum() - 1.0) <= 24 * 2.0 ** -53 * np.abs(c).sum()
        s = float(np.sum(F.solve_row(G, 1.0, b0=0.1, ridge=ridge) ** 2))
        assert prev is None or s <= prev * (1 + 1e-12)
        prev = s
    with pytest.raises(ValueError, match="ridge"):
        F.solve_row(G, 1.0, ridge=-1.0)


def test_sum_grams_is_the_same_for_any_batching():
    rng = np.random.default_rng(9)
    per = rng.standard_normal((7, 5, 5)) * 10.0 ** rng.integers(-6, 6, (7, 1, 1))
    whole = F.sum_grams(per)
    assert np.array_equal(whole, F.sum_grams([per[:2], per[2:3], torch.from_numpy(per[3:])]))
    acc = per[0].copy()
    for g in per[1:]:
        acc = acc + g
    assert np.array_equal(whole, acc)


# ---- fit_matrix: refusals that need no GPU ----

def _ddim(n):
    return coeffgen.ddim_vp_continuous(coeffgen.quadratic_time_grid(n))


def _no_gpu(monkeypatch):
    def boom():
        raise AssertionError("require_gpu was reached")
    monkeypatch.setattr(_lib, "require_gpu", boom)


def test_fit_matrix_refusals_come_before_the_gpu(monkeypatch, repo_root):
    _no_gpu(monkeypatch)
    teacher = _ddim(20)
    C, B, node = teacher
    init = coeffgen.ddim_vp_continuous(coeffgen.quadratic_time_grid(20)[::4])
    noise = torch.zeros(2, 3, 4, 4)
    model = lambda x, labels: x
    with pytest.raises(ValueError, match="stochastic"):
        F.fit_matrix(model, coeffgen.vp_euler(5, stochastic=True), teacher, noise)
    with pytest.raises(ValueError, match="stochastic"):
        F.fit_matrix(model, init, coeffgen.ddim_vp_continuous(coeffgen.quadratic_time_grid(20), eta=1.0), noise)
    off = (init[0], init[1], init[2].copy())
    off[2][3, 0] += 1e-4                                                       # no teacher node within t_tol of row 2's end
    with pytest.raises(ValueError, match="no node within"):
        F.fit_matrix(model, off, teacher, noise)
    F.match_nodes(off[2], node, [0, 1, 3, 4])                                  # the other rows still match
    for order in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="order"):
            F.fit_matrix(model, init, teacher, noise, order=order)
    with pytest.raises(ValueError, match="constraint"):
        F.fit_matrix(model, init, teacher, noise, constraint="sum")
    with pytest.raises(ValueError, match="rows"):
        F.fit_matrix(model, init, teacher, noise, rows=[5])
    with pytest.raises(ValueError, match="ridge"):
        F.fit_matrix(model, init, teacher, noise, ridge=-1e-3)
    with pytest.raises(ValueError, match="triple"):
        F.fit_matrix(model, (init[0], init[1]), teacher, noise)
    with pytest.raises(ValueError, match="fp32"):
        F.fit_matrix(model, init, teacher, noise.double())
    with pytest.raises(ValueError, match="multiple of 4"):
        F.fit_matrix(model, init, teacher, torch.zeros(2, 3, 5))
    big = _ddim(40)
    with pytest.raises(ValueError, match="supported columns"):
        F.fit_matrix(model, (big[0], big[1], big[2]), big, noise)              # row 30 has 31 columns: order is needed
    with pytest.raises(AssertionError, match="require_gpu was reached"):       # every check passed: the next thing is the GPU
        F.fit_matrix(model, init, teacher, noise, order=2)


def test_shipped_matrix_matches_the_quadratic_teacher_grid(repo_root):
    C, B, node = load_coeff_npz(repo_root / "weights" / "step_5_weight_00.npz")
    tnode = _ddim(20)[2]
    assert F.match_nodes(node, tnode, range(5)) == {k: 4 * (k + 1) for k in range(5)}
    assert np.abs(node[:, 0] - tnode[::4, 0]).max() > 1e-9                     # the stored times are not the grid's to 1e-9: hence t_tol = 1e-6
    with pytest.raises(ValueError, match="no node within"):
        F.match_nodes(node, tnode, range(5), t_tol=1e-9)
    # the constraint the fitter holds is the one the shipped matrices have
    assert np.abs(C.sum(1) - node[1:, 1]).max() <= 4e-16 and np.array_equal(B[:, 0], node[1:, 2]) and not np.any(B[:, 1:])


def test_oracle_fit_beats_ddim5_on_held_out_noise():
    """The reference arithmetic alone: sequential fitting of 5 rows to DDIM-20 on 16 images brings the held-out final error under DDIM-5's"""
    model = O.TwoPoint()
    teacher = _ddim(20)
    init = coeffgen.ddim_vp_continuous(coeffgen.quadratic_time_grid(20)[::4])
    rng = np.random.default_rng(3)
    fit_noise, held = rng.standard_normal((16, 3072)), rng.standard_normal((16, 3072))
    for order, bound in ((2, 0.75), (None, 0.62)):
        fitted = O.fit_sequential(model, init, teacher, fit_noise, order=order)
        assert np.abs(fitted[0].sum(1) - init[2][1:, 1]).max() <= 1e-12
        m_fit, m_init = O.final_mse(model, [fitted, init], teacher, held)
        assert m_fit / m_init <= bound, (order, m_fit, m_init)
