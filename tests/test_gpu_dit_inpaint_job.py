"""GPU tests of latent-space inpainting in the DiT generation job (``ValidateNaturalInference.generate_sharded(known_latents= / known_images=, mask=)``).
Three denoisers: a per-sample ELEMENTWISE stand-in (an element's trajectory then depends on that element alone, so the unknown elements must be the
unconditioned job's bytes), the small synthetic DiT engine (depth 2, hidden 128, input size 32) against a by-hand loop in this file that makes the same
forwards and calls the EXISTING step entry followed by natinf_known_blend_f32 -- the job's plumbing pinned without leaning on the new kernel -- and the
synthetic AutoencoderKL halves for the ``known_images`` form."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 27182
S, PER = 32, 4 * 32 * 32
COUNT = 10
LABELS = [(37 * i + 11) % 1000 for i in range(COUNT)]
ABAR = np.cumprod(1.0 - np.linspace(1e-4, 2e-2, 1000))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


class StandInDiT:
    """A denoiser from + - x / only whose output for an ELEMENT depends on that element of z, the sample's timestep and its class label alone
    (the stand-in of tests/test_gpu_dit_job.py): fp32 on the CPU.  [B, 8, S, S] like the DiT's learn_sigma output."""
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


def job(model, count=COUNT, labels=LABELS, **kw):
    from naturaldiffusion_amd import ValidateNaturalInference as V
    kw.setdefault("batch_size", 8)
    kw.setdefault("decode", False)
    return V.generate_sharded(count, labels, alg_name="ddpm", num_step=24, seed=SEED, model=model, **kw)


@pytest.fixture(scope="module")
def known():
    g = torch.Generator().manual_seed(3)
    kl = torch.randn(COUNT, 4, S, S, generator=g) * 0.7
    cells = torch.rand(COUNT, S, S, generator=g) > 0.5
    cells[:, 8:20, 5:17] = False                                  # a hole, and random cells around it
    cells[0, 0, :4] = torch.tensor([True, False, True, True])      # quads with mixed bytes in the first row
    return kl, cells


@pytest.fixture(scope="module")
def base(dev, known):
    """the unconditioned job and the inpainting job on the stand-in, batch size 8"""
    kl, cells = known
    plain = job(StandInDiT())[0]
    inp = job(StandInDiT(), known_latents=kl, mask=cells)[0]
    return plain, inp


def test_unknown_elements_are_the_unconditioned_jobs_known_elements_are_known(dev, known, base):
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd.coeff import load_coeff_npz
    kl, cells = known
    plain, inp = base
    node = load_coeff_npz(V.root_path / "results/ddpm/ddpm_024.npz")[2]
    assert node[24, 1] == 1.0 and node[24, 2] == 0.0            # why the known elements come back exactly: the last level is fp32(known * 1)
    m = cells[:, None].expand(-1, 4, -1, -1).to(dev)
    assert inp.shape == (COUNT, 4, S, S) and torch.isfinite(inp).all()
    assert 0 < int(m.sum()) < m.numel()
    assert torch.equal(inp[~m], plain[~m]), "an elementwise denoiser: the unknown elements never see the known ones"
    assert torch.equal(inp[m], kl.to(dev)[m])
    assert not torch.equal(inp, plain)
    # known_final="data" is the same here (alpha_N == 1)
    assert torch.equal(job(StandInDiT(), known_latents=kl, mask=cells, known_final="data")[0], inp)


def test_split_invariance(dev, known, base):
    kl, cells = known
    _, inp = base
    z3, lb, ix, img = job(StandInDiT(), known_latents=kl, mask=cells, batch_size=3)
    assert img is None and ix.tolist() == list(range(COUNT)) and lb.tolist() == LABELS
    assert torch.equal(z3, inp)
    full = torch.empty_like(inp)
    for r in range(2):
        z, lb, ix, _ = job(StandInDiT(), known_latents=kl, mask=cells, batch_size=3, rank=r, world=2)
        assert ix.tolist() == list(range(r, COUNT, 2))
        full[ix.to(dev)] = z
    assert torch.equal(full, inp)


def test_shared_row_and_mask_forms(dev, known, base):
    kl, cells = known
    _, inp = base
    # K = 1 equals its repetition, for the latents and for the mask
    one = job(StandInDiT(), known_latents=kl[:1], mask=cells[:1])[0]
    rep = job(StandInDiT(), known_latents=kl[:1].expand(COUNT, -1, -1, -1).contiguous(), mask=cells[:1].expand(COUNT, -1, -1).contiguous())[0]
    assert torch.equal(one, rep) and not torch.equal(one, inp)
    mixed = job(StandInDiT(), known_latents=kl, mask=cells[:1])[0]
    m0 = cells[:1, None].expand(COUNT, 4, -1, -1).to(dev)
    assert torch.equal(mixed[m0], kl.to(dev)[m0])
    # a [K, S, S] mask equals its 4-channel broadcast, bool or uint8
    four = job(StandInDiT(), known_latents=kl, mask=cells[:, None].expand(-1, 4, -1, -1).to(torch.uint8) * 255)[0]
    assert torch.equal(four, inp)
    # a genuinely per-channel mask: channel 0 alone
    ch = torch.zeros(COUNT, 4, S, S, dtype=torch.bool)
    ch[:, 0] = cells
    z = job(StandInDiT(), known_latents=kl, mask=ch)[0]
    plain = base[0]
    assert torch.equal(z[:, 0], inp[:, 0]) and torch.equal(z[:, 1:], plain[:, 1:])


def test_float_scale_equals_the_sequence(dev, known, base):
    """the default form (float cfg through the sampler's launch-wide slots) and the planned form (the caller's per-image tensors) give equal bytes on a
    batch-independent denoiser; a guidance interval composes"""
    kl, cells = known
    plain, inp = base
    seq = job(StandInDiT(), known_latents=kl, mask=cells, cfg_scale=[4.0] * COUNT)[0]
    assert torch.equal(seq, inp)
    m = cells[:, None].expand(-1, 4, -1, -1).to(dev)
    iv = job(StandInDiT(), known_latents=kl, mask=cells, guidance_interval=(200, 800))[0]
    iv_plain = job(StandInDiT(), guidance_interval=(200, 800))[0]
    assert torch.equal(iv[~m], iv_plain[~m]) and torch.equal(iv[m], kl.to(dev)[m]) and not torch.equal(iv, inp)


def test_without_the_arguments_neither_new_call_is_made(dev, base, monkeypatch):
    from naturaldiffusion_amd._lib import lib

    def poisoned(*a):
        raise AssertionError("an inpainting entry was called by a job without known data")
    monkeypatch.setattr(lib, "natinf_step_f32prod_inpaint", poisoned)
    monkeypatch.setattr(lib, "natinf_known_blend_f32", poisoned)
    assert torch.equal(job(StandInDiT())[0], base[0])
    assert torch.equal(job(StandInDiT(), cfg_scale=[4.0] * COUNT)[0], base[0])
    with pytest.raises(AssertionError):                           # and the poison is live: the inpainting job trips over it
        job(StandInDiT(), known_latents=torch.zeros(1, 4, S, S), mask=torch.ones(1, S, S, dtype=torch.bool))


# ------------------------------------------------------------------------------ the small synthetic engine
BATCH, N_ENG = 4, 5                                               # 5 images in batches of 4: a ragged last batch
ENG_LABELS = [207, 360, 387, 974, 88]


@pytest.fixture(scope="module")
def eng(dev):
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.dit import DiTEngine, flatten_state_dict
    P = D.make_params(2, 128, seed=11, grid=S // 2)
    return DiTEngine(flatten_state_dict(P, 2, 128), max_batch=2 * BATCH, depth=2, hidden=128, heads=2, input_size=S)


def by_hand(eng, dev, kl, mask_elems, scales=None):
    """The inpainting job restated with the existing entries: the same forwards, natinf_step_f32prod_noise (``scales`` None: cfg 4.0) or
    natinf_step_f32prod_noise_guided (every image guided, its own scale), then natinf_known_blend_f32 at level kk + 1; the first input is the blend at
    level 0."""
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd._lib import lib, ptr, stream_ptr
    from naturaldiffusion_amd.CIFAR10NaturalInference import philox_noise
    from naturaldiffusion_amd.coeff import load_coeff_npz
    from naturaldiffusion_amd.sampler import ValidateNI, known_schedule
    C, B, node = load_coeff_npz(V.root_path / "results/ddpm/ddpm_024.npz")
    tables, _ = V.skip_ddim_coeff(V.create_ddim_coeff(), 24)
    c1, c2 = np.asarray(tables[2])[::-1].astype(np.float32), np.asarray(tables[3])[::-1].astype(np.float32)
    levels = known_schedule(node, "mean")
    out = []
    for indices, labs in V.job_batches(N_ENG, BATCH, 0, 1, ENG_LABELS):
        n = len(indices)
        E = n * PER
        ni = ValidateNI(C, B, node, c1, c2, E, device=dev, seed=SEED, elems_per_image=PER)
        index = torch.tensor(indices, dtype=torch.int64, device=dev)
        lab = torch.tensor(labs, dtype=torch.int64, device=dev)
        nulls = torch.full((n,), 1000, dtype=torch.int64, device=dev)
        known = kl[indices].reshape(-1).to(dev)
        mask = mask_elems[indices].reshape(-1).to(dev)
        noise = philox_noise(indices, (4, S, S), SEED, dev, column=0)

        def blend(x, level):
            a, s, col = levels[level]
            o = torch.empty(E, device=dev)
            assert lib.natinf_known_blend_f32(ptr(x), ptr(o), ptr(known), ptr(mask), PER, PER, a, s, col, SEED, ptr(index), 0, 0, PER, E, stream_ptr()) == 0
            return o.view(n, 4, S, S)
        z = blend(noise.reshape(-1), 0)
        if scales is not None:
            cfg = torch.tensor([float(np.float32(scales[i])) for i in indices], dtype=torch.float32, device=dev)
            slots = torch.arange(n, dtype=torch.int32, device=dev)
        for kk in range(24):
            t = torch.full((n,), int(node[kk, 0]), dtype=torch.int32, device=dev)
            both = eng.forward(torch.cat([z, z]), torch.cat([t, t]), torch.cat([lab, nulls])).contiguous()
            if scales is None:
                un = ni.step(kk, z.reshape(-1), both[:n].contiguous(), both[n:].contiguous(), 4.0, PER, 2 * PER, noise=noise.reshape(-1), index=index)
            else:
                un = ni.step(kk, z.reshape(-1), both[:n], both[n:], cfg, PER, 2 * PER, noise=noise.reshape(-1), index=index, uncond_slot=slots, n_uncond=n)
            z = blend(un, kk + 1)
        out.append(z.clone())
    return torch.cat(out)


def test_job_on_the_engine_equals_the_by_hand_loop(dev, eng):
    g = torch.Generator().manual_seed(8)
    kl = torch.randn(N_ENG, 4, S, S, generator=g) * 0.7
    cells = torch.zeros(N_ENG, S, S, dtype=torch.bool)
    cells[:, :, :14] = True                                       # the left part known, the right part to be generated
    cells[1] = torch.rand(S, S, generator=g) > 0.6
    mask_elems = cells[:, None].expand(-1, 4, -1, -1).to(torch.uint8).contiguous()
    kw = dict(count=N_ENG, labels=ENG_LABELS, batch_size=BATCH)
    z = job(eng, known_latents=kl, mask=cells, **kw)[0]
    want = by_hand(eng, dev, kl, mask_elems)
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert np.array_equal(z.cpu().numpy(), want.cpu().numpy())
    m = mask_elems.bool().to(dev)
    assert torch.equal(z[m], kl.to(dev)[m])
    # the conditioning reaches the unknown region: a transformer mixes the tokens
    plain = job(eng, **kw)[0]
    assert not torch.equal(z[~m], plain[~m])
    # the planned form with per-image scales, every image guided: the same forwards (n + n rows), the guided entry + blend
    scales = [4.0, 2.5, 4.0, 3.0, 1.5]
    zs = job(eng, known_latents=kl, mask=cells, cfg_scale=scales, **kw)[0]
    assert np.array_equal(zs.cpu().numpy(), by_hand(eng, dev, kl, mask_elems, scales).cpu().numpy())
    assert not torch.equal(zs, z)


# ------------------------------------------------------------------------------ known_images: encoder, pixel mask, paste
def test_known_images_end_to_end(dev):
    from naturaldiffusion_amd.AnalyzeWeightedSumDegradation import preprocess
    from naturaldiffusion_amd.ValidateNaturalInference import latent_mask
    from naturaldiffusion_amd.synth import synthetic_vae_encoder_flat, synthetic_vae_flat
    from naturaldiffusion_amd.vae import VAEDecoder, VAEEncoder
    enc = VAEEncoder(synthetic_vae_encoder_flat(4, seed=2), max_batch=2, latent_ch=4, latent_res=S, device=dev)
    dec = VAEDecoder(synthetic_vae_flat(4, seed=1), max_batch=2, latent_ch=4, latent_res=S, device=dev)
    g = torch.Generator().manual_seed(12)
    R = 8 * S
    base_img = torch.randint(0, 256, (2, R // 8, R // 8, 3), generator=g, dtype=torch.uint8)
    u8 = base_img.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()            # blocky pictures, not white noise
    u8 = (u8.to(torch.int32) + torch.randint(0, 8, (2, R, R, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    mask_px = torch.ones(2, R, R, dtype=torch.bool)
    mask_px[0, 61:170, 83:200] = False                            # a hole that straddles cell borders
    mask_px[1, :, 131:] = False
    kw = dict(count=2, labels=[207, 88], batch_size=2, decode=True, decoder=dec, decode_batch=2)
    z, lb, ix, img = job(StandInDiT(), known_images=u8, mask=mask_px, encoder=enc, **kw)
    assert z.shape == (2, 4, S, S) and torch.isfinite(z).all() and img.shape == (2, R, R, 3) and img.dtype == torch.uint8 and not img.is_cuda
    # paste: the known pixels exactly where the pixel mask is set, the decoder's elsewhere
    assert torch.equal(img[mask_px], u8[mask_px])
    decoded = job(StandInDiT(), known_images=u8, mask=mask_px, encoder=enc, paste=False, **kw)
    assert torch.equal(decoded[0], z)
    assert torch.equal(img[~mask_px], decoded[3][~mask_px]) and not torch.equal(decoded[3][mask_px], u8[mask_px])
    # the latents are the known_latents job's, fed the posterior mean x 0.18215 and the reduced mask
    lat = enc.encode(preprocess(u8).to(dev), sample=False, scale=0.18215, index=[0, 1]).cpu()
    cells = latent_mask(mask_px, 1)
    assert 0 < int(cells.sum()) < int(latent_mask(mask_px, 0).sum()) < cells.numel()
    z2 = job(StandInDiT(), known_latents=lat, mask=cells, **dict(kw, decode=False))[0]
    assert torch.equal(z, z2)
    m = cells.bool()[:, None].expand(-1, 4, -1, -1)
    assert torch.equal(z.cpu()[m], lat[m])
    # the sink gets the pasted images; fp32 images encode to the same latents and are not pasted
    got = []
    job(StandInDiT(), known_images=u8, mask=mask_px, encoder=enc, image_sink=lambda im, i, l: got.append(im.cpu()), **kw)
    assert torch.equal(torch.cat(got), img)
    zf, _, _, imf = job(StandInDiT(), known_images=preprocess(u8), mask=mask_px, encoder=enc, **kw)
    assert torch.equal(zf, z) and torch.equal(imf, decoded[3])
