"""The SD3 job with latent-space inpainting (``SD3NaturalInference.sd_generate_sharded(known_latents= | known_images=, mask=, renoise=, mask_erode=)`` /
``sd_natural_inference_tx(sample_count=...)``, natinf_step_f16chain_inpaint) on the small MMDiT engine of test_gpu_sd3_guided_job.py: 2 layers, 2 heads,
grid 8, 13 text tokens, latent (16, 16, 16), five images in batches of two.  The yardstick is a loop written here over ``SD3NI`` and the engine."""
import zlib

import pytest
import torch

import vae_encoder_oracle as EO
from oracle import ni_oracle as O

pytestmark = pytest.mark.gpu

N, COUNT, SHAPE, TC = 2, 5, (16, 16, 16), 13
PER = 16 * 16 * 16
SEED = 10


def _embed(text):
    """(tokens [TC, 64], pooled [32]) fp16: a function of the string alone"""
    g = torch.Generator().manual_seed(zlib.crc32(text.encode()))
    return torch.randn(TC, 64, generator=g).half(), torch.randn(32, generator=g).half()


class Pipe:
    """the small engine pipe of test_gpu_sd3_guided_job.py; ``calls`` records the batch size of every ``transformer.forward``"""

    def __init__(self):
        from oracle import mmdit_oracle as M
        from naturaldiffusion_amd.mmdit import MMDiTEngine, flatten_state_dict
        cfg = dict(layers=2, heads=2, joint_dim=64, pooled_dim=32)
        P = dict(M.make_params(seed=1, pos_max=24, pos_base=8, **cfg))
        P["proj_out.weight"] = P["proj_out.weight"] * 0.2          # O(1) velocities: the 28-step fp16 chain stays well conditioned
        self.transformer = MMDiTEngine(flatten_state_dict(P, 8, **cfg), max_batch=2 * N, grid=8, ctx_tokens=TC, **cfg)
        self.calls = []
        forward = self.transformer.forward

        def recording(latents, timestep, text, pooled):
            self.calls.append(latents.shape[0])
            return forward(latents, timestep, text, pooled)
        self.transformer.forward = recording

        class Sched:
            def set_timesteps(self, k, device=None):
                self.timesteps, self.sigmas = O.sd3_sigma_schedule(k)
        self.scheduler = Sched()

    def encode_prompt(self, prompt, prompt_2=None, prompt_3=None, negative_prompt=""):
        pos, neg = [_embed(p) for p in prompt], [_embed("negative: " + negative_prompt)] * len(prompt)
        st = lambda rows, j: torch.stack([r[j] for r in rows]).cuda()
        return st(pos, 0), st(neg, 0), st(pos, 1), st(neg, 1)


@pytest.fixture(scope="module")
def pipe():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return Pipe()


@pytest.fixture(scope="module")
def data():
    """per-image known latents [5, 16, 16, 16] (fp16 values), a per-image cell mask: the left half known, plus one cell per image"""
    g = torch.Generator().manual_seed(21)
    known = (torch.randn(COUNT, *SHAPE, generator=g) * 0.8).half()
    cells = torch.zeros(COUNT, 16, 16, dtype=torch.uint8)
    cells[:, :, :8] = 1
    for i in range(COUNT):
        cells[i, 3 + i, 12] = 1
    return known, cells


def job(pipe, rank=0, world=1, **kw):
    from naturaldiffusion_amd import SD3NaturalInference as S
    pipe.calls.clear()
    return S.sd_generate_sharded(pipe, COUNT, N, rank, world, latent_shape=SHAPE, **kw)


def elems(cells):
    return cells[:, None].expand(-1, 16, -1, -1).bool()


@pytest.fixture(scope="module")
def fresh(pipe, data):
    """the inpainting job, per-image rows, renoise="fresh" -> (latents, forward sizes), computed once"""
    known, cells = data
    lat, idx = job(pipe, known_latents=known, mask=cells)
    assert idx.tolist() == list(range(COUNT)) and lat.dtype == torch.float16 and torch.isfinite(lat.float()).all()
    return lat.clone(), list(pipe.calls)


def by_hand(pipe, known, cells, renoise, scales=None):
    """the loop of the job written out: Philox noise by global index, ``SD3NI.first_input`` with the blend, a forward of [x; x] and the inpainting step
    with slots 0..n-1 (every image guided), the last step blending the mean"""
    from naturaldiffusion_amd.SD3NaturalInference import PROMPT, philox_noise_f16, root_path
    from naturaldiffusion_amd.sampler import SD3NI
    from naturaldiffusion_amd.shard import rank_batches
    W = O.load_sd3_csv(root_path / "weights/sd3_step_28_weight.csv")
    timesteps, sigmas = O.sd3_sigma_schedule(28)
    timesteps = timesteps.cuda()
    pe, ne, ppe, npe = pipe.encode_prompt([PROMPT] * N)
    mask_e = elems(cells).to(torch.uint8)
    outs = []
    for batch in rank_batches(COUNT, N, 0, 1):
        nb, rows = len(batch), torch.tensor(list(batch))
        noises = philox_noise_f16(batch, SHAPE, SEED, "cuda:0")
        ni = SD3NI(W, sigmas, noises.numel(), device="cuda:0", elems_per_image=PER)
        kw = dict(known=known[rows].reshape(-1).cuda(), mask=mask_e[rows].reshape(-1).contiguous().cuda(), seed=SEED, index=rows.cuda(), renoise=renoise)
        cfg = torch.tensor([7.0 if scales is None else scales[i] for i in batch], dtype=torch.float32).cuda()
        slots = torch.arange(nb, dtype=torch.int32).cuda()
        flat = noises.reshape(-1)
        x = ni.first_input(flat, **kw)
        for kk in range(28):
            xs = x.view(noises.shape)
            v = pipe.transformer.forward(torch.cat([xs, xs]), timesteps[kk].expand(2 * nb), torch.cat([pe[:nb], ne[:nb]]), torch.cat([ppe[:nb], npe[:nb]]))
            mean, x = ni.step(kk, x, v[:nb].contiguous().reshape(-1), v[nb:].contiguous().reshape(-1), flat, want_next=kk < 27, cfg=cfg, uncond_slot=slots,
                              n_uncond=nb, sample_elems=PER, blend_mean=kk == 27, **kw)
        outs.append(mean.view(noises.shape).clone())
    return torch.cat(outs)


@pytest.mark.parametrize("renoise", ["fresh", "same"])
def test_job_is_the_loop_written_by_hand(pipe, data, fresh, renoise):
    known, cells = data
    lat = fresh[0] if renoise == "fresh" else job(pipe, known_latents=known, mask=cells, renoise="same")[0]
    want = by_hand(pipe, known, cells, renoise)
    assert torch.isfinite(want.float()).all()
    assert torch.equal(lat.view(torch.int16), want.view(torch.int16))


def test_known_elements_are_known_and_the_rest_is_generated(pipe, data, fresh):
    known, cells = data
    lat, calls = fresh
    assert calls == [4] * 28 + [4] * 28 + [2] * 28
    m = elems(cells).cuda()
    assert torch.equal(lat[m].view(torch.int16), known.cuda()[m].view(torch.int16))
    default, _ = job(pipe)
    assert not torch.equal(lat[~m], default[~m])                                   # the known half steers the other half
    same, _ = job(pipe, known_latents=known, mask=cells, renoise="same")
    assert torch.equal(same[m], known.cuda()[m]) and not torch.equal(same[~m], lat[~m])


def test_split_invariance(pipe, data, fresh):
    """one rank ([0,1] [2,3] [4]) against two ranks ([0,2] [4] | [1,3]): the known elements are the same bytes; the rest agrees to the engine's own batch
    dependence (test_gpu_sd3_shard.py's bf16-level bound, 2e-2 of the largest latent), image 4 -- alone in its batch both times -- and a repeated split
    byte for byte"""
    known, cells = data
    lat1 = fresh[0]
    whole = torch.empty_like(lat1)
    for world in (1, 2):
        for r in range(world):
            lat, idx = job(pipe, r, world, known_latents=known, mask=cells)
            assert idx.tolist() == list(range(r, COUNT, world))
            whole[idx.cuda()] = lat
        if world == 1:
            assert torch.equal(whole, lat1)
    m = elems(cells).cuda()
    assert torch.equal(whole[m], lat1[m]) and torch.equal(whole[4], lat1[4])
    err = ((whole.float() - lat1.float()).abs().max() / lat1.float().abs().max()).item()
    print("two ranks vs one, max rel:", err)
    assert err <= 2e-2, err
    again, _ = job(pipe, 1, 2, known_latents=known, mask=cells)
    assert torch.equal(again, whole[torch.tensor([1, 3]).cuda()])


def test_shared_row_and_per_image_forms_agree(pipe, data):
    known, cells = data
    k1, c1 = known[:1], cells[:1]
    shared, _ = job(pipe, known_latents=k1, mask=c1)
    expanded, _ = job(pipe, known_latents=k1.expand(COUNT, -1, -1, -1), mask=c1.expand(COUNT, -1, -1))
    assert torch.equal(shared, expanded)
    # a latent-element mask and the cell mask it spells out are the same job
    elem, _ = job(pipe, known_latents=k1, mask=elems(c1))
    assert torch.equal(shared, elem)
    m = elems(c1).expand(COUNT, -1, -1, -1).cuda()
    assert torch.equal(shared[m], k1.expand(COUNT, -1, -1, -1).cuda()[m])


def test_float_scale_is_the_uniform_sequence(pipe, data, fresh):
    known, cells = data
    lat, _ = job(pipe, known_latents=known, mask=cells, cfg_scale=[7.0] * COUNT)
    assert torch.equal(lat, fresh[0]) and pipe.calls == fresh[1]
    a, _ = job(pipe, known_latents=known, mask=cells, cfg_scale=3.5)
    b, _ = job(pipe, known_latents=known, mask=cells, cfg_scale=[3.5] * COUNT)
    assert torch.equal(a, b) and not torch.equal(a, fresh[0])
    # per-image scales compose: an unguided image takes no null-prompt sequence
    scales = [7, 1, 3.5, 1, 7]
    mixed, _ = job(pipe, known_latents=known, mask=cells, cfg_scale=scales)
    assert pipe.calls == [3] * 28 + [3] * 28 + [2] * 28
    m = elems(cells).cuda()
    assert torch.equal(mixed[m], known.cuda()[m]) and torch.isfinite(mixed.float()).all()


def test_without_the_arguments_neither_new_symbol_is_called(pipe, monkeypatch):
    from naturaldiffusion_amd import sampler
    before, _ = job(pipe)
    called = []

    class Spy:
        def __getattr__(self, name):
            if name in ("natinf_known_blend_f16", "natinf_step_f16chain_inpaint"):
                called.append(name)
            return getattr(sampler._lib.lib, name)
    monkeypatch.setattr(sampler, "lib", Spy())
    lat, _ = job(pipe)
    planned, _ = job(pipe, cfg_scale=[7.0] * COUNT)
    assert called == [] and torch.equal(lat, before) and torch.equal(planned, before)
    known = torch.zeros(1, *SHAPE)
    job(pipe, known_latents=known, mask=torch.ones(1, 16, 16, dtype=torch.uint8))
    assert called.count("natinf_known_blend_f16") == 3 and called.count("natinf_step_f16chain_inpaint") == 3 * 28     # and the spy does see them


def test_known_images_end_to_end(pipe):
    """128 x 128 images through a synthetic 16-channel encoder at latent_res 16: the job equals the job run on the latents ``encode`` gives"""
    from naturaldiffusion_amd.AnalyzeWeightedSumDegradation import preprocess
    from naturaldiffusion_amd.vae import VAEEncoder, flatten_encoder_state_dict
    scale, shift = 1.5305, 0.0609

    class Vae:
        class config:
            scaling_factor, shift_factor, latent_channels = scale, shift, 16
    pipe.vae = Vae()
    pipe.natinf_vae_encoder = enc = VAEEncoder(flatten_encoder_state_dict(EO.make_params(16, seed=4), 16), max_batch=N, latent_ch=16, latent_res=16)
    try:
        g = torch.Generator().manual_seed(31)
        coarse = torch.randint(0, 256, (COUNT, 16, 16, 3), generator=g, dtype=torch.uint8)
        images = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()          # [5, 128, 128, 3] uint8
        px = torch.zeros(1, 128, 128, dtype=torch.bool)
        px[:, :, :72] = True                                                                   # nine cells known, eight after one ring of erosion
        lat, idx = job(pipe, known_images=images, mask=px)
        assert idx.tolist() == list(range(COUNT)) and torch.isfinite(lat.float()).all()
        kl = torch.cat([enc.encode(preprocess(images[s:s + N]).cuda(), sample=False, scale=scale, shift=shift) for s in range(0, COUNT, N)])
        assert tuple(kl.shape) == (COUNT, *SHAPE) and kl.dtype == torch.float32
        cells = torch.zeros(1, 16, 16, dtype=torch.uint8)
        cells[:, :, :8] = 1
        want, _ = job(pipe, known_latents=kl.cpu(), mask=cells)
        assert torch.equal(lat, want)
        m = elems(cells).expand(COUNT, -1, -1, -1).cuda()
        assert torch.equal(lat[m], kl.half()[m])
        # fp32 NCHW images in [-1, 1] on one rank of two: the rank's own rows are encoded, in one chunk; a shared image is encoded alone
        encode = lambda rows: enc.encode(preprocess(images[rows]).cuda(), sample=False, scale=scale, shift=shift).cpu()
        lat_r, idx_r = job(pipe, 1, 2, known_images=preprocess(images), mask=px)
        rows_r = torch.zeros(COUNT, *SHAPE)
        rows_r[[1, 3]] = encode([1, 3])
        want_r, _ = job(pipe, 1, 2, known_latents=rows_r, mask=cells)
        assert idx_r.tolist() == [1, 3] and torch.equal(lat_r, want_r)
        one, _ = job(pipe, known_images=images[2:3], mask=px)
        assert torch.equal(one, job(pipe, known_latents=encode([2]), mask=cells)[0])
        assert torch.equal(job(pipe, known_images=images, mask=px, mask_erode=0)[0][:, :, :, 8], kl.half()[:, :, :, 8])   # no erosion: nine columns known
    finally:
        del pipe.vae, pipe.natinf_vae_encoder


def test_entry_point_forwards_the_arguments(pipe, data):
    from naturaldiffusion_amd import SD3NaturalInference as S
    known, cells = data
    kw = dict(known_latents=known, mask=cells, renoise="same")
    lat, idx = job(pipe, 0, 2, **kw)
    (lat_e, idx_e), = S.sd_natural_inference_tx(pipe=pipe, n=N, decode=False, weight_names=("sd3_step_28_weight.csv",), rank=0, world=2,
                                                 sample_count=COUNT, device="cuda:0", **kw)
    assert torch.equal(lat_e, lat) and idx_e.tolist() == idx.tolist() == [0, 2, 4]
    assert not torch.equal(lat, job(pipe, 0, 2, known_latents=known, mask=cells)[0])           # renoise reaches the step
    with pytest.raises(ValueError, match="sample_count"):
        S.sd_natural_inference_tx(pipe=pipe, n=N, decode=False, **kw)
