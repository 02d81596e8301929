"""The DiT generation job on the host (no GPU): the batch planner ``ValidateNaturalInference.job_batches`` (sharding by global
image index, label by global index), which shipped DDPM / DDIM matrices inject noise after a step, and the yardstick the GPU
tests of the job lean on -- the CPU restatement of the Validate loop (oracle.ni_oracle.validate_ni) fed Philox column noises
against the classical ancestral sampler fed the same draws."""
import numpy as np
import pytest
import torch

from naturaldiffusion_amd.coeff import is_stochastic, load_coeff_npz
from oracle import ni_oracle as O
from oracle import philox_oracle as P

DEMO = [207, 360, 387, 974, 88, 979, 417, 279]
SEED = 0


def column_noise(indices, elems_per_image, seed, column):
    """float32 [len(indices), elems_per_image] as natinf_randn_philox_col_f32 keys it: counter = (index lo, index hi, element
    quad, column), key = seed (the construction of tests/test_ni_stochastic_host.py)."""
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


# ------------------------------------------------------------------------------ 1. the planner
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("batch_size", [1, 3, 8, 32])
@pytest.mark.parametrize("sample_count", [0, 1, 20, 101])
def test_job_batches_partition(world, batch_size, sample_count):
    from naturaldiffusion_amd.ValidateNaturalInference import job_batches
    seen, label_of = [], {}
    for rank in range(world):
        batches = job_batches(sample_count, batch_size, rank, world)
        mine = [i for idx, _ in batches for i in idx]
        assert mine == list(range(rank, sample_count, world))                 # rank r owns r, r+world, ...
        assert all(len(idx) == batch_size for idx, _ in batches[:-1])          # only the last batch is ragged
        assert all(0 < len(idx) <= batch_size and len(idx) == len(lb) for idx, lb in batches)
        for idx, lb in batches:
            for i, l in zip(idx, lb):
                label_of[i] = l
        seen += mine
    assert sorted(seen) == list(range(sample_count))                          # every index exactly once
    assert all(label_of[i] == DEMO[i % 8] for i in range(sample_count))


def test_job_batches_label_is_a_function_of_the_global_index():
    from naturaldiffusion_amd.ValidateNaturalInference import job_batches
    full = [(7 * i) % 1000 for i in range(20)]
    for labels, want in ((None, lambda i: DEMO[i % 8]), (full, lambda i: full[i]), ([5, 999, 0], lambda i: [5, 999, 0][i % 3]),
                         (torch.tensor([3, 4]), lambda i: 3 + i % 2), (np.array([9]), lambda i: 9)):
        ref = None
        for world, batch in ((1, 8), (2, 3), (1, 20), (3, 32), (8, 1)):
            got = {}
            for rank in range(world):
                for idx, lb in job_batches(20, batch, rank, world, labels):
                    assert all(isinstance(v, int) for v in idx + lb)
                    got.update(zip(idx, lb))
            assert got == {i: want(i) for i in range(20)}
            ref = got if ref is None else ref
            assert got == ref
    assert job_batches(8, 8)[0] == (list(range(8)), DEMO)                     # the demo's row


def test_job_batches_refusals():
    from naturaldiffusion_amd.ValidateNaturalInference import job_batches
    for bad in ([1000], [-1], [5, 1000, 7], [2 ** 31]):
        with pytest.raises(ValueError):
            job_batches(4, 2, labels=bad)                                     # 1000 is the null class
    with pytest.raises(ValueError):
        job_batches(4, 2, labels=[])
    with pytest.raises(ValueError):
        job_batches(4, 2, labels=[1, 2, 3, 4, 5])                             # more labels than images
    with pytest.raises(ValueError):
        job_batches(4, 0)
    with pytest.raises(ValueError):
        job_batches(-1, 2)
    with pytest.raises(ValueError):
        job_batches(4, 2, rank=2, world=2)


# ------------------------------------------------------------------------------ 2. which matrices are stochastic
@pytest.mark.parametrize("rel,want", [("results/ddpm/ddpm_018", True), ("results/ddpm/ddpm_024", True),
                                      ("results/ddpm/ddpm_sympy_018", True), ("results/ddpm/ddpm_sympy_024", True),
                                      ("results/ddim/ddim_018", False), ("results/ddim/ddim_024", False)])
def test_is_stochastic_on_the_dit_matrices(repo_root, rel, want):
    C, B, node = load_coeff_npz(repo_root / f"{rel}.npz")
    n = C.shape[0]
    assert B.shape == (n, n + 1) and is_stochastic(B) is want
    assert all(np.count_nonzero(B[k, k + 2:]) == 0 for k in range(n))         # row k uses eps_0 .. eps_{k+1}
    if rel.endswith("ddpm_024") or rel.endswith("ddpm_sympy_024"):
        assert np.count_nonzero(B) == 300
    if rel.endswith("ddim_024"):
        assert np.count_nonzero(B[-1]) == 0                                   # a row without a noise term is legal


# ------------------------------------------------------------------------------ 3. the yardstick of the GPU tests
def label_eps_model(labels, cfg=4.0):
    """fused-eps stand-in that depends on the class label, from + - x / only: the oracle's analytic model
    plus a label-scaled bump, for the conditional and the null (1000) half, fused like the reference fuses them."""
    base = O.analytic_eps_model()
    lab = torch.as_tensor(labels, dtype=torch.float32)

    def half(z, t, y):
        w = (y / 4000.0 - 0.125)[:, None, None, None]
        return base(z, t) + w * (z / (1.0 + z * z))

    def eps_fn(z, t):
        return O.cfg_fuse(half(z, t, lab), half(z, t, torch.full_like(lab, 1000.0)), cfg)
    return eps_fn


@pytest.mark.parametrize("name", ["ddpm_sympy_024", "ddpm_024", "ddpm_018"])
def test_restatement_with_philox_columns_matches_the_ancestral_sampler(repo_root, name):
    """validate_ni fed eps_j = Philox(seed, image index, column j) == the classical DDPM skip sampler fed the same draws,
    within the bound tests/test_ni_oracle.py::test_validate_original_vs_natural uses for this pair."""
    C, B, node = load_coeff_npz(repo_root / f"results/ddpm/{name}.npz")
    n = B.shape[0]
    idx = [0, 5, 2 ** 33 + 1]
    eps = [torch.from_numpy(column_noise(idx, 4096, SEED, j)).view(3, 4, 32, 32) for j in range(n + 1)]
    eps_fn = label_eps_model([207, 88, 999])
    a = O.validate_ni(eps_fn, eps[0], eps[1:], C, B, node)
    b = O.validate_original(eps_fn, eps[0], eps[1:], n, stochastic=True)
    rel = float((a - b).abs().max() / b.abs().max())
    print(f"{name}: NI restatement vs ancestral sampler, Philox columns: {rel:.3e}")
    assert torch.isfinite(b).all() and rel < 5e-6, rel
