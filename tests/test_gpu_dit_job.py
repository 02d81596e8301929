"""GPU tests of the DiT generation job: the Validate-form step with in-kernel noise (natinf_step_f32prod_noise, include/natinf.h),
``sampler.ValidateNI(seed=...)`` and ``ValidateNaturalInference.generate_sharded``.  The step regenerates eps_j (j >= 1) from
Philox(seed, global image index, column j) in registers; natinf_randn_philox_col_f32 returns the same normals, so the slab
path (natinf_step_f32prod on a slab filled through ``philox_noise(column=j)``) and the CPU restatement fed those columns are
reproduced byte for byte."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from naturaldiffusion_amd.coeff import load_coeff_npz
from oracle import ni_oracle as O

SEED = 20240
DEMO = [207, 360, 387, 974, 88, 979, 417, 279]
ABAR = np.cumprod(1.0 - np.linspace(1e-4, 2e-2, 1000))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def matrix(repo_root, name):
    return load_coeff_npz(repo_root / ("results/%s/%s.npz" % (name.split("_")[0], name)))


def c1c2(n):
    from naturaldiffusion_amd import ValidateNaturalInference as V
    tables, _ = V.skip_ddim_coeff(V.create_ddim_coeff(), n)
    return np.asarray(tables[2])[::-1].astype(np.float32), np.asarray(tables[3])[::-1].astype(np.float32)


def columns(indices, shape, n_cols, dev, seed=SEED):
    from naturaldiffusion_amd.CIFAR10NaturalInference import philox_noise
    return [philox_noise(indices, shape, seed, dev, column=j) for j in range(n_cols)]


class StandInDiT:
    """A denoiser from + - x / only whose output for a sample depends on that sample's z, timestep and
    class label alone: fp32 on the CPU, so the same function drives the kernel path and the CPU restatement.  [B, 8, S, S]
    like the DiT's learn_sigma output; channels 4-7 are what the step must not read."""
    max_batch = 1 << 20

    def __init__(self, input_size=32):
        self.input_size = input_size

    @staticmethod
    def eps(z, t, y):
        z = z.detach().to("cpu", torch.float32)
        a = torch.from_numpy((1.0 - ABAR[t.detach().cpu().long().numpy()]).astype(np.float32))[:, None, None, None]
        w = (y.detach().to("cpu", torch.float32) / 4000.0 - 0.125)[:, None, None, None]
        z3 = z * 3.0
        return z * a + 0.1 * (z3 / (1.0 + z3 * z3)) + w * (z / (1.0 + z * z))

    def forward(self, z, t, y):
        e = self.eps(z, t, y)
        return torch.cat([e, torch.full_like(e, 1e9)], 1).to(z.device)


def fused_eps_fn(labels, cfg=4.0):
    """the CPU twin of one CFG step through ``StandInDiT``: eps_fn(z, int timestep) of oracle.ni_oracle.validate_ni"""
    lab = torch.as_tensor(labels, dtype=torch.int64)

    def eps_fn(z, t):
        tt = torch.full((len(lab),), int(t), dtype=torch.int32)
        return O.cfg_fuse(StandInDiT.eps(z, tt, lab), StandInDiT.eps(z, tt, torch.full_like(lab, 1000)), cfg)
    return eps_fn


# ------------------------------------------------------------------------------ 5. the step against the slab path
INDEX_FORMS = ("tensor", "first", "pair")


def index_form(form, n):
    """-> (global indices, the ``index`` argument of ValidateNI.step)"""
    if form == "tensor":
        idx = [(2 ** 33 + 5 if i == 1 else 977 * i + 3) for i in range(n)] if n > 1 else [2 ** 33 + 5]
        return idx, idx
    if form == "first":
        return [1000 + i for i in range(n)], 1000
    return [2 ** 34 + 7 + 3 * i for i in range(n)], (2 ** 34 + 7, 3)


@pytest.mark.parametrize("name", ["ddpm_024", "ddpm_sympy_024", "ddpm_018", "ddim_024"])
def test_step_equals_the_slab_path(dev, repo_root, name):
    """every row of the matrix, dense and sparse, 1 / 3 / 37 images of 4,096 elements and 2 of 16,384, with and without uncond,
    contiguous and 8-channel-strided cond, the three index forms: z_next and hist_x0[k] of natinf_step_f32prod_noise are the
    bytes of natinf_step_f32prod on the slab ``philox_noise(column=j)`` filled"""
    from naturaldiffusion_amd.sampler import ValidateNI
    C, B, node = matrix(repo_root, name)
    n = B.shape[0]
    c1, c2 = c1c2(n)
    g = torch.Generator().manual_seed(n)
    checked = 0
    for n_img, se in ((1, 4096), (3, 4096), (37, 4096), (2, 16384)):
        E = n_img * se
        z = torch.randn(E, generator=g).to(dev)
        cond8 = torch.randn(n_img, 2 * se, generator=g).to(dev)
        unc8 = torch.randn(n_img, 2 * se, generator=g).to(dev)
        cond4, unc4 = cond8[:, :se].contiguous(), unc8[:, :se].contiguous()
        hist0 = torch.randn(n, E, generator=g).to(dev)
        for form in INDEX_FORMS:
            idx, arg = index_form(form, n_img)
            if form == "tensor":
                arg = torch.tensor(idx, dtype=torch.int64, device=dev)
            slab = torch.stack([c.reshape(-1) for c in columns(idx, (se,), n + 1, dev)])
            for dense in (False, True):
                old = ValidateNI(C, B, node, c1, c2, E, device=dev, dense=dense)
                new = ValidateNI(C, B, node, c1, c2, E, device=dev, dense=dense, seed=SEED)
                assert new.hist_eps is None
                old.hist_eps = slab
                for k in range(n):
                    for with_uncond, strided in itertools.product((True, False), (False, True)):
                        old.hist_x0.copy_(hist0); new.hist_x0.copy_(hist0)
                        c, u, st = (cond8, unc8, 2 * se) if strided else (cond4, unc4, se)
                        u = u if with_uncond else None
                        a = old.step(k, z, c, u, 4.0, se, st)
                        b = new.step(k, z, c, u, 4.0, se, st, noise=slab[0], index=arg)
                        assert torch.equal(a, b), (name, n_img, se, form, dense, k, with_uncond, strided)
                        assert torch.equal(old.hist_x0, new.hist_x0), (name, n_img, se, form, dense, k, "hist_x0")
                        checked += 1
    assert checked == 4 * 3 * 2 * n * 4
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ 6. trajectory against the CPU restatement
@pytest.mark.parametrize("name", ["ddpm_sympy_024", "ddim_024"])
def test_trajectory_equals_the_cpu_restatement(dev, repo_root, name):
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd.sampler import ValidateNI
    C, B, node = matrix(repo_root, name)
    n, S = B.shape[0], 32
    idx = [3, 4, 5, 2 ** 33 + 9, 6]
    labels = [207, 0, 999, 417, 88]
    per = 4 * S * S
    eps = columns(idx, (4, S, S), n + 1, dev)
    ref = O.validate_ni(fused_eps_fn(labels), eps[0].cpu(), [e.cpu() for e in eps[1:]], C, B, node, return_all=True)
    c1, c2 = c1c2(n)
    ni = ValidateNI(C, B, node, c1, c2, len(idx) * per, device=dev, seed=SEED, elems_per_image=per)
    model = StandInDiT()
    index = torch.tensor(idx, dtype=torch.int64, device=dev)
    lab = torch.tensor(labels, device=dev)
    nulls = torch.full((len(idx),), 1000, device=dev)
    z = eps[0]
    for k in range(n):
        t = torch.full((len(idx),), int(node[k, 0]), dtype=torch.int32, device=dev)
        cond, uncond = V._cond_uncond(model, z, t, lab, nulls)
        z = ni.step(k, z.reshape(-1), cond, uncond, 4.0, per, 2 * per, noise=eps[0].reshape(-1), index=index).view(-1, 4, S, S)
        assert np.array_equal(z.cpu().numpy(), ref[k + 1].numpy()), f"{name}: z_{k + 1} differs from the restatement"


# ------------------------------------------------------------------------------ 7. split invariance of the job
@pytest.mark.parametrize("alg", ["ddpm_sympy", "ddim"])
def test_job_is_invariant_to_the_split(dev, alg):
    from naturaldiffusion_amd import ValidateNaturalInference as V
    model = StandInDiT()
    labels = [(37 * i + 11) % 1000 for i in range(20)]
    kw = dict(alg_name=alg, num_step=24, seed=SEED, decode=False, model=model)
    one, l1, i1, img = V.generate_sharded(20, labels, batch_size=8, **kw)
    assert img is None and torch.equal(i1, torch.arange(20)) and l1.tolist() == labels and one.shape == (20, 4, 32, 32)
    assert one.dtype == torch.float32 and one.is_cuda and torch.isfinite(one).all()
    whole, _, _, _ = V.generate_sharded(20, labels, batch_size=20, **kw)
    assert torch.equal(whole, one)
    full = torch.empty_like(one)
    for r in range(2):
        z, lb, ix, _ = V.generate_sharded(20, labels, batch_size=3, rank=r, world=2, **kw)
        assert ix.tolist() == list(range(r, 20, 2)) and lb.tolist() == [labels[i] for i in ix.tolist()]
        full[ix.to(dev)] = z
    assert torch.equal(full, one)
    # labels=None: the reference's demo row on indices 0-7; a different label is a different image, a different seed too
    demo, ld, _, _ = V.generate_sharded(11, None, batch_size=4, **kw)
    assert ld.tolist() == [DEMO[i % 8] for i in range(11)]
    same, _, _, _ = V.generate_sharded(8, DEMO, batch_size=8, **kw)
    assert torch.equal(same, demo[:8])
    assert not torch.equal(demo[0], one[0])
    other, _, _, _ = V.generate_sharded(8, DEMO, batch_size=8, **dict(kw, seed=SEED + 1))
    assert not torch.equal(other, same)
    # and the job is the restatement: image by image what oracle.ni_oracle.validate_ni gives for these indices and labels
    C, B, node = load_coeff_npz(V.root_path / ("results/%s/%s_024.npz" % (alg.replace("_sympy", ""), alg)))
    eps = columns(range(8), (4, 32, 32), 25, dev)
    ref = O.validate_ni(fused_eps_fn(DEMO), eps[0].cpu(), [e.cpu() for e in eps[1:]], C, B, node)
    assert np.array_equal(same.cpu().numpy(), ref.numpy())


# ------------------------------------------------------------------------------ 8. the job on the real engine
def small_engine(S, max_batch, seed=11):
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.dit import DiTEngine, flatten_state_dict
    P = D.make_params(2, 128, seed=seed, grid=S // 2)
    return P, DiTEngine(flatten_state_dict(P, 2, 128), max_batch=max_batch, depth=2, hidden=128, heads=2, input_size=S)


def slab_path(V, eng, C, B, node, indices, labels, S, dev):
    """today's path for one batch: the slab ValidateNI, natinf_step_f32prod, the slab filled from philox_noise(column=j)"""
    from naturaldiffusion_amd.sampler import ValidateNI
    n, N, per = len(indices), B.shape[0], 4 * S * S
    c1, c2 = c1c2(N)
    ni = ValidateNI(C, B, node, c1, c2, n * per, device=dev)
    for j, e in enumerate(columns(indices, (4, S, S), N + 1, dev)):
        ni.hist_eps[j].copy_(e.reshape(-1))
    z = ni.hist_eps[0].clone().view(n, 4, S, S)
    lab = torch.tensor(labels, dtype=torch.int64, device=dev)
    nulls = torch.full((n,), 1000, dtype=torch.int64, device=dev)
    for k in range(N):
        t = torch.full((n,), int(node[k, 0]), dtype=torch.int32, device=dev)
        cond, uncond = V._cond_uncond(eng, z, t, lab, nulls)
        z = ni.step(k, z.reshape(-1), cond.contiguous(), uncond.contiguous(), 4.0, per, 8 * S * S).view(n, 4, S, S)
    return z.clone()


@pytest.mark.parametrize("S", [32, 64])
def test_job_on_the_engine_equals_the_slab_path(dev, S):
    """(a) generate_sharded == the same batches through the slab path with the same forwards, byte for byte (the engine is
    run-to-run deterministic for a fixed batch shape: checked first)"""
    from naturaldiffusion_amd import ValidateNaturalInference as V
    P, eng = small_engine(S, 8)
    g = torch.Generator().manual_seed(S)
    x = torch.randn(8, 4, S, S, generator=g).to(dev)
    t = torch.linspace(999.0, 3.0, 8).to(dev)
    y = torch.tensor([1, 1000, 207, 5, 1000, 999, 0, 88]).to(dev)
    assert torch.equal(eng(x, t, y), eng(x, t, y)), "the DiT engine is not run-to-run deterministic"
    labels = [(91 * i + 7) % 1000 for i in range(7)]
    for alg in ("ddpm_sympy", "ddim"):
        C, B, node = load_coeff_npz(V.root_path / ("results/%s/%s_024.npz" % (alg.replace("_sympy", ""), alg)))
        z, lb, ix, img = V.generate_sharded(7, labels, alg_name=alg, batch_size=4, seed=SEED, decode=False, model=eng)
        assert z.shape == (7, 4, S, S) and img is None and torch.isfinite(z).all()
        want = torch.cat([slab_path(V, eng, C, B, node, idx, lab, S, dev) for idx, lab in V.job_batches(7, 4, labels=labels)])
        assert torch.equal(z, want), alg


@pytest.mark.parametrize("S,n_img", [(32, 4), (64, 2)])
@pytest.mark.parametrize("alg", ["ddim", "ddpm_sympy"])
def test_job_on_the_engine_against_the_dit_oracle(dev, alg, S, n_img):
    """(b) generate_sharded on the bf16 engine against validate_ni driven by the fp32 DiT oracle and the kernel's own noise
    columns: within the 5e-2 tests/test_gpu_dit.py::test_validate_natural_inference_end_to_end uses for this comparison"""
    from oracle import dit_oracle as D
    from naturaldiffusion_amd import ValidateNaturalInference as V
    P, eng = small_engine(S, 2 * n_img)
    labels = DEMO[:n_img]
    z, _, ix, _ = V.generate_sharded(n_img, None, alg_name=alg, batch_size=n_img, seed=SEED, decode=False, model=eng)
    lab, nulls = torch.tensor(labels), torch.full((n_img,), 1000)

    def eps_fn(x, t):
        tt = torch.full((n_img,), float(t))
        return O.cfg_fuse(D.forward(P, x, tt, lab, 2)[:, :4], D.forward(P, x, tt, nulls, 2)[:, :4], 4.0)
    C, B, node = load_coeff_npz(V.root_path / ("results/%s/%s_024.npz" % (alg.replace("_sympy", ""), alg)))
    eps = [e.cpu() for e in columns(ix.tolist(), (4, S, S), 25, dev)]
    ref = O.validate_ni(eps_fn, eps[0], eps[1:], C, B, node)
    rel = ((z.cpu() - ref).abs().max() / ref.abs().max()).item()
    print(f"generate_sharded({alg}_024, {8 * S}x{8 * S}) on the engine vs the DiT oracle: {rel:.3e}")
    assert rel <= 5e-2, rel


# ------------------------------------------------------------------------------ 9. decode
def test_decode_and_image_sink(dev):
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd.synth import synthetic_vae_flat
    from naturaldiffusion_amd.vae import VAEDecoder
    vae = VAEDecoder(synthetic_vae_flat(4, seed=1), max_batch=3, latent_ch=4, latent_res=32, device=dev)
    kw = dict(alg_name="ddim", batch_size=4, seed=SEED, model=StandInDiT(), decoder=vae, decode_batch=3)
    z, lb, ix, img = V.generate_sharded(7, None, **kw)
    assert img.shape == (7, 256, 256, 3) and img.dtype == torch.uint8 and not img.is_cuda
    want = []
    for s in range(0, 7, 3):
        x = vae(z[s:s + 3] / 0.18215).detach().float()
        want.append(((((x.clamp(-1, 1) + 1) * 0.5) * 255 + 0.5).clamp(0, 255)).to(torch.uint8).permute(0, 2, 3, 1).cpu())
    want = torch.cat(want)
    assert torch.equal(img, want) and len(torch.unique(want)) > 16
    got = []

    def sink(u8, indices, labels):
        assert u8.is_cuda and u8.dtype == torch.uint8 and u8.shape == (len(indices), 256, 256, 3) and len(indices) <= 3
        got.append((u8.cpu(), list(indices), list(labels)))
    z2, _, _, none = V.generate_sharded(7, None, image_sink=sink, **kw)
    assert none is None and torch.equal(z2, z)
    assert [i for _, idx, _ in got for i in idx] == list(range(7))                       # every index exactly once
    assert [l for _, _, lab in got for l in lab] == [DEMO[i % 8] for i in range(7)]
    assert torch.equal(torch.cat([u for u, _, _ in got]), want)
    assert V.generate_sharded(7, None, **dict(kw, decode=False))[3] is None


# ------------------------------------------------------------------------------ 10. the large-batch shape
def test_xl2_batch_32(dev):
    """DiT-XL/2 (synthetic weights), 32 images = forwards of 64 samples: finite, the workspace natinf_dit_workspace_bytes
    predicts for 64 samples, no launch error"""
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd._lib import lib
    from naturaldiffusion_amd.dit import DiTEngine, flatten_state_dict, XL2
    from naturaldiffusion_amd.synth import synthetic_dit_state_dict
    eng = DiTEngine(flatten_state_dict(synthetic_dit_state_dict(), XL2["depth"], XL2["hidden"]), max_batch=64, **XL2)
    assert eng.workspace_bytes == lib.natinf_dit_workspace_bytes(eng._h, 64) > lib.natinf_dit_workspace_bytes(eng._h, 16) > 0
    z, lb, ix, img = V.generate_sharded(32, None, alg_name="ddim", batch_size=32, seed=SEED, decode=False, model=eng)
    torch.cuda.synchronize()
    assert z.shape == (32, 4, 32, 32) and torch.isfinite(z).all() and float(z.abs().max()) > 0
    assert lb.tolist() == [DEMO[i % 8] for i in range(32)] and ix.tolist() == list(range(32))


# ------------------------------------------------------------------------------ 11. refusals
def test_entry_refusals(dev):
    from naturaldiffusion_amd._lib import lib, ptr
    E = 16
    x = torch.zeros(E, device=dev)
    h = torch.zeros(4 * E, device=dev)
    ic = torch.tensor([0], dtype=torch.int32, device=dev)
    vc = torch.tensor([0.5], dtype=torch.float32, device=dev)
    vb = torch.tensor([0.5, 0.5, 0.5, 0.5], dtype=torch.float32, device=dev)
    rows = {name: torch.tensor(v, dtype=torch.int32, device=dev) for name, v in
            dict(ok=[0, 1, 2], no0=[1, 2], above=[0, 1, 3], negative=[-1, 1], long=[0, 1, 2, 2]).items()}
    torch.cuda.synchronize()

    def step(E=E, se=8, st=8, noise=x, row="ok", n_b=None, k=1, idx_b=True, val_b=True, n_c=0, idx_c=None):
        ib = rows[row]
        return lib.natinf_step_f32prod_noise(ptr(x), ptr(x), ptr(x), 4.0, se, st, ptr(h), ptr(noise), ptr(x), ptr(idx_c), ptr(vc), n_c, 1.0,
                                             ptr(ib) if idx_b else None, ptr(vb) if val_b else None, len(ib) if n_b is None else n_b,
                                             k, 1.0, 0.5, SEED, None, 0, 1, E, None)
    assert step(E=14) == -1 and step(E=0) == -1                              # E % 4
    assert step(se=6, st=8) == -1 and step(se=0) == -1                        # sample_elems % 4
    assert step(E=12, se=8) == -1                                             # E % sample_elems
    assert step(E=4 * 2 ** 32, se=4 * 2 ** 32, st=4 * 2 ** 32) == -1          # quad count does not fit counter word 2
    assert step(st=4) == -1                                                   # stride below the sample
    assert step(noise=None) == -1                                             # the row names column 0
    assert step(row="above") == -1 and step(row="ok", k=0) == -1              # eps_j exists from step j-1 on
    assert step(row="negative") == -1 and step(row="long") == -1
    assert step(idx_b=False) == -1 and step(val_b=False) == -1 and step(n_b=-1) == -1      # terms_ok
    assert step(n_c=1, idx_c=None) == -1 and step(k=-1) == -1
    torch.cuda.synchronize()
    assert torch.equal(x, torch.zeros_like(x)) and torch.equal(h, torch.zeros_like(h))      # nothing was launched
    assert step() == 0 and step(noise=None, row="no0") == 0 and step(n_b=0) == 0 and step(n_b=0, noise=None) == 0
    assert step(n_c=1, idx_c=ic) == 0
    torch.cuda.synchronize()


def test_sampler_refusals(dev, repo_root):
    from naturaldiffusion_amd.sampler import ValidateNI
    C, B, node = matrix(repo_root, "ddpm_024")
    c1, c2 = c1c2(24)
    per, E = 4096, 2 * 4096
    z = torch.zeros(E, device=dev)
    with pytest.raises(ValueError):
        ValidateNI(C, B, node, c1, c2, E, device=dev, elems_per_image=per)              # elems_per_image without a seed
    for bad in (0, 6, 3 * 1024):
        with pytest.raises(ValueError):
            ValidateNI(C, B, node, c1, c2, E, device=dev, seed=1, elems_per_image=bad)
    old = ValidateNI(C, B, node, c1, c2, E, device=dev)
    assert old.hist_eps.shape == (25, E)
    with pytest.raises(ValueError):
        old.step(0, z, z, z, 4.0, per, per, noise=z)                                    # slab sampler, seeded call
    with pytest.raises(ValueError):
        old.step(0, z, z, z, 4.0, per, per, index=0)
    ni = ValidateNI(C, B, node, c1, c2, E, device=dev, seed=1, elems_per_image=per)
    assert ni.hist_eps is None
    with pytest.raises(ValueError):
        ni.step(0, z, z, z, 4.0, per, per)                                              # seeded sampler, hist_eps-style call
    with pytest.raises(ValueError):
        ni.step(0, z, z, z, 4.0, 2 * per, 2 * per, noise=z)                             # not the constructor's image size
    for bad in (z[:per], z.double(), z.cpu(), torch.zeros(2 * E, device=dev)[::2]):
        with pytest.raises(ValueError):
            ni.step(0, z, z, z, 4.0, per, per, noise=bad)
    for bad in (torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64),
                torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)[::2]):
        with pytest.raises(ValueError):
            ni.step(0, z, z, z, 4.0, per, per, noise=z, index=bad)
    for good in (None, 5, (5, 2), [2 ** 40, 1], torch.tensor([7, 2 ** 35], dtype=torch.int64, device=dev)):
        ni.step(0, z, z, z, 4.0, per, per, noise=z, index=good)
    torch.cuda.synchronize()
