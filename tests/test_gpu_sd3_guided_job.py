"""The SD3 job with per-image prompts, CFG scales and a guidance interval (``SD3NaturalInference.sd_generate_sharded`` /
``sd_natural_inference_tx(sample_count=...)``, natinf_step_f16chain_guided) on a small MMDiT engine: 2 layers, 2 heads, grid 8, 13 text tokens,
latent (16, 16, 16), five images in batches of two.  ``encode_prompt`` returns embeddings that are a deterministic function of each prompt string."""
import zlib

import numpy as np
import pytest
import torch

from oracle import ni_oracle as O

pytestmark = pytest.mark.gpu

N, COUNT, SHAPE, TC = 2, 5, (16, 16, 16), 13
A, B = "a red fox in the snow", "a lighthouse at dusk"
SCALES = [7, 1, 3.5, 1, 7]
PROMPTS = [A, B, A, A, A]


def _embed(text):
    """(tokens [TC, 64], pooled [32]) fp16: a function of the string alone"""
    g = torch.Generator().manual_seed(zlib.crc32(text.encode()))
    return torch.randn(TC, 64, generator=g).half(), torch.randn(32, generator=g).half()


class Pipe:
    """the small engine pipe of test_gpu_sd3_shard.py with per-prompt embeddings; ``calls`` records the batch size of every ``transformer.forward``"""

    def __init__(self):
        from oracle import mmdit_oracle as M
        from naturaldiffusion_amd.mmdit import MMDiTEngine, flatten_state_dict
        cfg = dict(layers=2, heads=2, joint_dim=64, pooled_dim=32)
        P = dict(M.make_params(seed=1, pos_max=24, pos_base=8, **cfg))
        P["proj_out.weight"] = P["proj_out.weight"] * 0.2          # O(1) velocities: the 28-step fp16 chain stays well conditioned
        self.transformer = MMDiTEngine(flatten_state_dict(P, 8, **cfg), max_batch=2 * N, grid=8, ctx_tokens=TC, **cfg)
        self.calls, self.encoded = [], []
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
        self.encoded.append(list(prompt))
        pos, neg = [_embed(p) for p in prompt], [_embed("negative: " + negative_prompt)] * len(prompt)
        st = lambda rows, j: torch.stack([r[j] for r in rows]).cuda()
        return st(pos, 0), st(neg, 0), st(pos, 1), st(neg, 1)


@pytest.fixture(scope="module")
def pipe():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return Pipe()


def job(pipe, rank=0, world=1, **kw):
    from naturaldiffusion_amd import SD3NaturalInference as S
    pipe.calls.clear()
    pipe.encoded.clear()
    return S.sd_generate_sharded(pipe, COUNT, N, rank, world, latent_shape=SHAPE, **kw)


@pytest.fixture(scope="module")
def default(pipe):
    """the job with none of the new arguments -> (latents, the forward sizes it made)"""
    lat, idx = job(pipe)
    assert idx.tolist() == list(range(COUNT)) and torch.isfinite(lat.float()).all()
    return lat.clone(), list(pipe.calls)


def test_default_arguments_are_the_untouched_path(pipe, default):
    from naturaldiffusion_amd.SD3NaturalInference import PROMPT
    lat0, calls0 = default
    assert calls0 == [4] * 28 + [4] * 28 + [2] * 28                   # every step a forward of 2n sequences
    lat, _ = job(pipe, prompts=None, negative_prompt="", cfg_scale=7.0, guidance_interval=None)
    assert torch.equal(lat, lat0) and pipe.calls == calls0 and pipe.encoded == [[PROMPT] * N]      # encoded once, for n prompts


def test_uniform_scale_sequence_is_the_default_form_byte_for_byte(pipe, default):
    """cfg_scale=[7.0]*5: the planned path with the forward shapes of the default form; the kernel's identity rule makes the latents the same bytes"""
    lat0, calls0 = default
    lat, _ = job(pipe, cfg_scale=[7.0] * COUNT)
    assert pipe.calls == calls0
    assert torch.equal(lat, lat0)


def test_unguided_job_matches_a_loop_on_n_sequences(pipe):
    """cfg_scale=1.0 with an interval that holds no sigma == cfg_scale=[1.0]*5 == a loop written here: ``engine.forward`` on the n text sequences
    and the CPU fp16 restatement of the unguided step (f = x - sig*v_text, ``sd3_weighted_mean``, the next flow input)"""
    from naturaldiffusion_amd.SD3NaturalInference import PROMPT, philox_noise_f16
    from naturaldiffusion_amd.shard import rank_batches
    lat_a, _ = job(pipe, cfg_scale=1.0, guidance_interval=(1.5, 2.0))
    calls_a = list(pipe.calls)
    lat_b, _ = job(pipe, cfg_scale=[1.0] * COUNT)
    assert calls_a == pipe.calls == [2] * 28 + [2] * 28 + [1] * 28    # n sequences a step, never 2n
    assert torch.equal(lat_a, lat_b)
    W = O.load_sd3_csv(pipe_root() / "weights/sd3_step_28_weight.csv")
    timesteps, sigmas = O.sd3_sigma_schedule(28)
    pe, _, ppe, _ = pipe.encode_prompt([PROMPT] * N)
    outs = []
    for batch in rank_batches(COUNT, N, 0, 1):
        nb = len(batch)
        noises = philox_noise_f16(batch, SHAPE, 10, "cuda:0").cpu()
        seq, mean = [], torch.zeros_like(noises)
        for kk in range(28):
            sig = sigmas[kk]
            x = sig * noises + (1 - sig) * mean
            v = pipe.transformer.forward(x.cuda(), timesteps[kk].cuda().expand(nb), pe[:nb], ppe[:nb]).cpu()
            assert v.dtype == torch.float16
            seq.append(x - sig * v)
            mean = O.sd3_weighted_mean(seq, W)
        outs.append(mean)
    want = torch.cat(outs)
    assert torch.isfinite(want.float()).all()
    assert np.array_equal(lat_a.cpu().numpy().view(np.uint16), want.numpy().view(np.uint16))


def pipe_root():
    from naturaldiffusion_amd.SD3NaturalInference import root_path
    return root_path


@pytest.fixture(scope="module")
def interval():
    _, sigmas = O.sd3_sigma_schedule(28)
    return float(sigmas[19]), float(sigmas[8])                        # steps 8..19, both ends on a sigma of the schedule


def predicted_calls(batches, interval):
    from naturaldiffusion_amd.SD3NaturalInference import sd_guidance_plan
    _, sigmas = O.sd3_sigma_schedule(28)
    calls = []
    for batch in batches:
        guided, slots, _ = sd_guidance_plan(sigmas, 28, [SCALES[i] for i in batch], interval)
        g = sum(s >= 0 for s in slots)
        calls += [len(batch) + g if on else len(batch) for on in guided]
    return calls


def test_mixed_job(pipe, interval):
    """scales [7, 1, 3.5, 1, 7], two prompts, guidance at steps 8..19: the forwards are the plan's, one rank and two ranks agree, a repeated split is the
    same bytes, and swapping the two prompts changes exactly the images that carry them"""
    from naturaldiffusion_amd.shard import rank_batches
    kw = dict(prompts=PROMPTS, cfg_scale=SCALES, guidance_interval=interval)
    lat1, idx1 = job(pipe, **kw)
    want = predicted_calls(rank_batches(COUNT, N, 0, 1), interval)
    assert want == [2] * 8 + [3] * 12 + [2] * 8 + [2] * 8 + [3] * 12 + [2] * 8 + [1] * 8 + [2] * 12 + [1] * 8
    assert pipe.calls == want
    assert pipe.encoded == [[A, B], [A, A], [A]]                      # once per batch, that batch's prompts
    assert idx1.tolist() == list(range(COUNT)) and torch.isfinite(lat1.float()).all()
    whole = torch.empty_like(lat1)
    for r in range(2):
        lat, idx = job(pipe, r, 2, **kw)
        assert idx.tolist() == list(range(r, COUNT, 2))
        assert pipe.calls == predicted_calls(rank_batches(COUNT, N, r, 2), interval)
        whole[idx.cuda()] = lat
    err = ((whole.float() - lat1.float()).abs().max() / lat1.float().abs().max()).item()
    print("two ranks vs one, max rel:", err)
    assert err <= 2e-2, err
    again, _ = job(pipe, 1, 2, **kw)
    assert torch.equal(again, whole[torch.tensor([1, 3]).cuda()])
    # the guidance does something: the mixed job is not the default one, nor the unguided one
    assert not torch.equal(lat1, job(pipe, prompts=PROMPTS)[0]) and not torch.equal(lat1, job(pipe, prompts=PROMPTS, cfg_scale=[1.0] * COUNT)[0])
    # swap the prompts of images 0 and 1: those two change, the other batches are the same bytes
    swapped, _ = job(pipe, prompts=[B, A, A, A, A], cfg_scale=SCALES, guidance_interval=interval)
    changed = [not torch.equal(swapped[i], lat1[i]) for i in range(COUNT)]
    assert changed == [True, True, False, False, False], changed


def test_entry_point_forwards_the_new_arguments(pipe, interval):
    from naturaldiffusion_amd import SD3NaturalInference as S
    kw = dict(prompts=PROMPTS, negative_prompt="blurry", cfg_scale=SCALES, guidance_interval=interval)
    lat, idx = job(pipe, 0, 2, **kw)
    (lat_e, idx_e), = S.sd_natural_inference_tx(pipe=pipe, n=N, decode=False, weight_names=("sd3_step_28_weight.csv",), rank=0, world=2,
                                                 sample_count=COUNT, device="cuda:0", **kw)
    assert torch.equal(lat_e, lat) and idx_e.tolist() == idx.tolist() == [0, 2, 4]
    assert not torch.equal(lat, job(pipe, 0, 2, **{**kw, "negative_prompt": ""})[0])      # the negative prompt reaches encode_prompt (images 0, 2, 4 are guided)
