"""GPU tests of the DiT generation job's guidance arguments (``ValidateNaturalInference.generate_sharded(cfg_scale=<sequence>,
guidance_interval=...)``) on a small synthetic engine (depth 2, hidden 128, 2 heads, input size 32, built for 2 x batch).
Expected latents come from hand-rolled loops in this file that make the same engine forwards and call the EXISTING step entry
(natinf_step_f32prod_noise through ``ValidateNI.step(cfg=<float>)``), once per group of images that share a scale, so the job's
plumbing is pinned without leaning on the new kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 5150
S, PER, BATCH, COUNT = 32, 4 * 32 * 32, 4, 5                   # 5 images in batches of 4: a ragged last batch
LABELS = [207, 360, 387, 974, 88]
INTERVAL = (200, 800)
SCALES = [4, 1, 4, 1, 2]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(dev):
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.dit import DiTEngine, flatten_state_dict
    P = D.make_params(2, 128, seed=11, grid=S // 2)
    return DiTEngine(flatten_state_dict(P, 2, 128), max_batch=2 * BATCH, depth=2, hidden=128, heads=2, input_size=S)


@pytest.fixture(scope="module")
def coeff():
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd.coeff import load_coeff_npz
    C, B, node = load_coeff_npz(V.root_path / "results/ddpm/ddpm_024.npz")
    tables, _ = V.skip_ddim_coeff(V.create_ddim_coeff(), B.shape[0])
    return C, B, node, np.asarray(tables[2])[::-1].astype(np.float32), np.asarray(tables[3])[::-1].astype(np.float32)


class Counting:
    """the engine behind a wrapper that records the row count of every forward"""

    def __init__(self, eng):
        self.eng, self.max_batch, self.input_size, self.rows = eng, eng.max_batch, eng.input_size, []

    def forward(self, z, t, y):
        self.rows.append(int(z.shape[0]))
        return self.eng.forward(z, t, y)


def job(model, **kw):
    from naturaldiffusion_amd import ValidateNaturalInference as V
    return V.generate_sharded(COUNT, LABELS, alg_name="ddpm", num_step=24, batch_size=kw.pop("batch_size", BATCH), seed=SEED, decode=False, model=model, **kw)


def sampler(coeff, n, dev):
    from naturaldiffusion_amd.sampler import ValidateNI
    C, B, node, c1, c2 = coeff
    return ValidateNI(C, B, node, c1, c2, n * PER, device=dev, seed=SEED, elems_per_image=PER)


def by_hand(eng, coeff, dev, scales=None, interval=None, batch_size=BATCH, rank=0, world=1):
    """The job restated with the existing step entry.  ``scales`` None: the default form -- [z; z] every step, one launch with cfg 4.0.
    Otherwise the planned form: at a guided step one forward of [z; z[G]], then natinf_step_f32prod_noise once per group of images
    that share a scale (its own sampler: its images' history) with ``uncond=None`` for the unguided ones; at every other step one forward
    of the n conditional samples and ``uncond=None`` for every group."""
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd.CIFAR10NaturalInference import philox_noise
    node = coeff[2]
    out = []
    for indices, labs in V.job_batches(COUNT, batch_size, rank, world, LABELS):
        n = len(indices)
        index = torch.tensor(indices, dtype=torch.int64, device=dev)
        lab = torch.tensor(labs, dtype=torch.int64, device=dev)
        noise = philox_noise(indices, (4, S, S), SEED, dev, column=0)
        z = noise
        if scales is None:
            ni = sampler(coeff, n, dev)
            nulls = torch.full((n,), 1000, dtype=torch.int64, device=dev)
            for kk in range(24):
                t = torch.full((n,), int(node[kk, 0]), dtype=torch.int32, device=dev)
                both = eng.forward(torch.cat([z, z]), torch.cat([t, t]), torch.cat([lab, nulls]))
                z = ni.step(kk, z.reshape(-1), both[:n].contiguous(), both[n:].contiguous(), 4.0, PER, 2 * PER, noise=noise.reshape(-1), index=index).view(n, 4, S, S)
            out.append(z.clone())
            continue
        sc = [float(np.float32(scales[i])) for i in indices]
        G = [i for i, s in enumerate(sc) if s != 1.0]
        row_of = {i: r for r, i in enumerate(G)}
        groups = {}
        for i, s in enumerate(sc):
            groups.setdefault(s, []).append(i)
        groups = {s: (imgs, torch.tensor(imgs, device=dev), sampler(coeff, len(imgs), dev)) for s, imgs in groups.items()}
        for kk in range(24):
            ts = int(node[kk, 0])
            inside = bool(G) and (interval is None or interval[0] <= ts <= interval[1])
            m = n + len(G) if inside else n
            t = torch.full((m,), ts, dtype=torch.int32, device=dev)
            if inside:
                zz = torch.cat([z, z[torch.tensor(G, device=dev)]])
                both = eng.forward(zz, t, torch.cat([lab, torch.full((len(G),), 1000, dtype=torch.int64, device=dev)]))
            else:
                both = eng.forward(z, t, lab)
            z_next = torch.empty_like(z)
            for s, (imgs, sel, ni) in groups.items():
                unc = both[n:][torch.tensor([row_of[i] for i in imgs], device=dev)].contiguous() if inside and s != 1.0 else None
                zs = ni.step(kk, z[sel].reshape(-1).contiguous(), both[:n][sel].contiguous(), unc, s, PER, 2 * PER,
                             noise=noise[sel].reshape(-1).contiguous(), index=index[sel].contiguous())
                z_next[sel] = zs.view(len(imgs), 4, S, S)
            z = z_next
        out.append(z.clone())
    return torch.cat(out)


def test_default_call_makes_the_calls_it_always_made(dev, eng, coeff):
    """new arguments at their defaults: the latents of the hand-rolled [z; z] loop on the scalar entry, byte for byte, and forwards of 2n"""
    count = Counting(eng)
    z, lb, ix, img = job(count)
    assert z.shape == (COUNT, 4, S, S) and img is None and lb.tolist() == LABELS and ix.tolist() == list(range(COUNT))
    assert count.rows == [8] * 24 + [2] * 24
    want = by_hand(eng, coeff, dev)
    assert torch.isfinite(want).all() and np.array_equal(z.cpu().numpy(), want.cpu().numpy())
    # an explicit 4.0 is the default call
    assert torch.equal(job(eng, cfg_scale=4.0)[0], z)


def test_forward_sizes_follow_the_plan(dev, eng, coeff):
    from naturaldiffusion_amd.ValidateNaturalInference import guidance_plan
    node = coeff[2]
    guided, _, _ = guidance_plan(node, 24, [4.0] * BATCH, INTERVAL)
    assert 0 < sum(guided) < 24
    count = Counting(eng)
    job(count, guidance_interval=INTERVAL)
    assert count.rows == [2 * BATCH if g else BATCH for g in guided] + [2 if g else 1 for g in guided]
    assert count.rows.count(2 * BATCH) == sum(guided) and count.rows.count(BATCH) == 24 - sum(guided)
    # per-image scales: forwards of n + |G| at every step -- [4, 1, 4, 1] is 4 + 2, [2] is 1 + 1
    count = Counting(eng)
    job(count, cfg_scale=SCALES)
    assert count.rows == [6] * 24 + [2] * 24
    # both: n + |G| inside, n outside
    count = Counting(eng)
    job(count, cfg_scale=SCALES, guidance_interval=INTERVAL)
    assert count.rows == [6 if g else 4 for g in guided] + [2 if g else 1 for g in guided]
    # every image unguided: never an unconditional sample
    count = Counting(eng)
    job(count, cfg_scale=1.0, guidance_interval=(0, 999))
    assert count.rows == [4] * 24 + [1] * 24


@pytest.mark.parametrize("scales,interval", [(4.0, INTERVAL), (SCALES, None), (SCALES, INTERVAL)], ids=["interval", "per_image", "both"])
def test_guided_job_bytes(dev, eng, coeff, scales, interval):
    """the job == the same forwards with the existing entry applied per group of images that share a scale"""
    z = job(eng, cfg_scale=scales, guidance_interval=interval)[0]
    table = [scales] * COUNT if isinstance(scales, float) else scales
    want = by_hand(eng, coeff, dev, scales=table, interval=interval)
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert np.array_equal(z.cpu().numpy(), want.cpu().numpy())
    assert not torch.equal(z, job(eng)[0]), "the guidance arguments changed nothing"


def test_resharding(dev, eng):
    """world = 2 returns, rank by rank, the images of the world = 1 job.  With batch_size 1 every image is alone in its forwards under either
    split (2 rows at a step that guides it, else 1), so the engine's forwards have the same row counts and the latents are equal byte for byte.
    With batch_size 4 the row counts differ between the splits (the engine picks GEMM variants by row count): those are compared within the 5e-2
    tests/test_gpu_dit.py uses for the engine against its oracle."""
    kw = dict(cfg_scale=SCALES, guidance_interval=INTERVAL)
    one, l1, i1, _ = job(eng, batch_size=1, **kw)
    four = job(eng, **kw)[0]
    for bs, whole, exact in ((1, one, True), (BATCH, four, False)):
        full = torch.empty_like(whole)
        for r in range(2):
            z, lb, ix, _ = job(eng, batch_size=bs, rank=r, world=2, **kw)
            assert ix.tolist() == list(range(r, COUNT, 2)) and lb.tolist() == [LABELS[i] for i in ix.tolist()]
            full[ix.to(dev)] = z
        if exact:
            assert np.array_equal(full.cpu().numpy(), whole.cpu().numpy())
        else:
            rel = float((full - whole).abs().max() / whole.abs().max())
            print(f"world 2 vs world 1 at batch {bs}: rel err {rel:.3e}")
            assert rel <= 5e-2, rel
    # image i's scale follows its global index: image 1 (scale 1) is the unguided image, whatever the split
    alone = job(eng, batch_size=1, cfg_scale=1.0, guidance_interval=(0, 999))[0]
    assert torch.equal(alone[1], one[1]) and not torch.equal(alone[0], one[0])
