"""Host-side checks of per-image guidance on the SD3 form: the argument errors of natinf_step_f16chain_guided that are decided before
any device is touched (include/natinf.h; dummy pointers are never dereferenced by the argument check, and there is no GPU here), the
pure planning functions of the SD3 job (``SD3NaturalInference.sd_guidance_plan`` / ``job_prompts``) and the job's argument checks, which
are made before the job asks for a GPU.  ``SD3NI`` needs a GPU to be constructed: the refusals of ``SD3NI.step`` are in
tests/test_gpu_sd3_guided_step.py."""
import numpy as np
import pytest
import torch

from oracle import ni_oracle as O

D = 4096                                                      # a non-NULL dummy pointer
ARGS = ("x", "v_text", "v_null", "cfg_image", "uncond_slot", "n_uncond", "sample_elems", "noise", "hist", "mean_out", "x_next",
        "idx", "val", "n_terms", "c_diag", "w_total", "k", "sig", "sig_next", "oms_next", "flags", "E", "stream")
GOOD = dict(x=D, v_text=D, v_null=D, cfg_image=D, uncond_slot=D, n_uncond=2, sample_elems=16, noise=D, hist=D, mean_out=D, x_next=D,
            idx=D, val=D, n_terms=1, c_diag=1.0, w_total=1.5, k=1, sig=0.5, sig_next=0.25, oms_next=0.75, flags=0, E=32, stream=None)


def call(**kw):
    from naturaldiffusion_amd._lib import lib
    a = {**GOOD, **kw}
    return lib.natinf_step_f16chain_guided(*[a[name] for name in ARGS])


def test_guided_entry_argument_errors():
    """every refusal is NATINF_EINVAL (-1) before a device is asked for anything"""
    for name in ("x", "v_text", "hist"):
        assert call(**{name: None}) == -1, name
    assert call(cfg_image=None) == -1 and call(uncond_slot=None) == -1                  # the two per-image arrays
    assert call(n_uncond=-1) == -1                                                       # a negative row count
    assert call(n_uncond=1, v_null=None) == -1 and call(n_uncond=2, v_null=None) == -1   # rows announced, none given
    assert call(sample_elems=12, E=24) == -1 and call(sample_elems=4, E=32) == -1        # sample_elems % 8
    assert call(sample_elems=0) == -1 and call(sample_elems=-16) == -1
    assert call(sample_elems=24, E=32) == -1 and call(sample_elems=64, E=32) == -1       # E % sample_elems
    # and every refusal of natinf_step_f16chain
    assert call(E=28) == -1 and call(E=0) == -1 and call(E=-32) == -1                    # E % 8, E > 0
    assert call(k=-1) == -1
    assert call(n_terms=-1) == -1 and call(idx=None) == -1 and call(val=None) == -1      # terms_ok
    assert call(noise=None) == -1                                                        # x_next wanted, no noise to mix
    assert call(flags=2) == -1 and call(flags=3) == -1 and call(flags=-1) == -1          # unknown flag bits


@pytest.fixture(scope="module")
def sigmas():
    return O.sd3_sigma_schedule(28)[1]                         # fp32 [29], descending, the last one 0


def test_plan_slots_compact_the_guided_images(sigmas):
    from naturaldiffusion_amd.SD3NaturalInference import sd_guidance_plan
    guided, slots, scales = sd_guidance_plan(sigmas, 28, [7, 1, 3.5, 1], None)
    assert slots == [0, -1, 1, -1] and scales == [7.0, 1.0, 3.5, 1.0] and guided == [True] * 28
    for n in (1, 4, 7):
        assert sd_guidance_plan(sigmas, 28, [7.0] * n, None) == ([True] * 28, list(range(n)), [7.0] * n)
    # the scale is the fp32 value the kernel multiplies by
    assert sd_guidance_plan(sigmas, 28, [0.1], None)[2] == [float(np.float32(0.1))]
    # the plan takes the schedule as a tensor, an array or a list
    for s in (sigmas.numpy(), [float(v) for v in sigmas]):
        assert sd_guidance_plan(s, 28, [7, 1], (0.3, 0.8)) == sd_guidance_plan(sigmas, 28, [7, 1], (0.3, 0.8))


def test_plan_every_scale_one_means_no_guided_step(sigmas):
    from naturaldiffusion_amd.SD3NaturalInference import sd_guidance_plan
    for interval in (None, (0.0, 1.0), (0.3, 0.8)):
        guided, slots, _ = sd_guidance_plan(sigmas, 28, [1.0, 1, 1.0], interval)
        assert slots == [-1, -1, -1] and guided == [False] * 28


def test_plan_interval_is_inclusive_on_the_fp32_sigmas(sigmas):
    from naturaldiffusion_amd.SD3NaturalInference import sd_guidance_plan
    sg = [float(sigmas[kk]) for kk in range(28)]               # the fp32 values, exact as doubles
    assert sigmas.dtype == torch.float32 and len(set(sg)) == 28 and sg == sorted(sg, reverse=True) and sg[0] == 1.0
    plan = lambda lo, hi: sd_guidance_plan(sigmas, 28, [2.0], (lo, hi))[0]
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(2)))       # the next fp32 above / below
    down = lambda v: float(np.nextafter(np.float32(v), np.float32(-1)))
    # an interval between two neighbouring sigmas holds none: nothing is guided; nor does one above the schedule
    assert plan(up(sg[10]), down(sg[9])) == [False] * 28
    assert plan(1.5, 2.0) == [False] * 28
    # some: exactly the kk whose sigma lies in it
    want = [0.3 <= v <= 0.8 for v in sg]
    assert 0 < sum(want) < 28
    guided, slots, _ = sd_guidance_plan(sigmas, 28, [7.0] * 3, (0.3, 0.8))
    assert guided == want and slots == [0, 1, 2]
    # a sigma as either end is inside; one fp32 step, or a double's breadth, past it is outside
    a, b = sg[17], sg[5]                                       # a < b
    assert plan(a, b) == [5 <= kk <= 17 for kk in range(28)]
    assert plan(up(a), b) == [5 <= kk <= 16 for kk in range(28)] == plan(a + 1e-12, b)
    assert plan(a, down(b)) == [6 <= kk <= 17 for kk in range(28)] == plan(a, b - 1e-12)
    assert plan(a, a) == [kk == 17 for kk in range(28)]
    # the last sigma the loop uses is sigmas[27] > 0; sigmas[28] == 0 belongs to no step
    assert plan(0.0, 0.0) == [False] * 28
    # an interval over everything is the plan without one
    assert sd_guidance_plan(sigmas, 28, [2.0], (0.0, 1.0)) == sd_guidance_plan(sigmas, 28, [2.0], None)


def test_plan_refuses_wrong_lengths(sigmas):
    from naturaldiffusion_amd.SD3NaturalInference import sd_guidance_plan
    for bad in ((0.5,), (0.2, 0.5, 0.8), (), (0.8, 0.3)):
        with pytest.raises(ValueError):
            sd_guidance_plan(sigmas, 28, [7.0], bad)
    with pytest.raises(ValueError):
        sd_guidance_plan(sigmas[:20], 28, [7.0], None)         # fewer sigmas than steps


def test_job_prompts_follow_the_global_index():
    from naturaldiffusion_amd.SD3NaturalInference import PROMPT, job_prompts
    from naturaldiffusion_amd.shard import rank_batches
    assert job_prompts(None, 3) == [PROMPT] * 3 and job_prompts("a dog", 2) == ["a dog"] * 2 and job_prompts("a dog", 0) == []
    table = ["prompt %d" % (i % 5) for i in range(11)]
    assert job_prompts(table, 11) == table and job_prompts(tuple(table), 11) == table
    for bad in (table[:10], table + ["x"], [], table[:10] + [3]):
        with pytest.raises(ValueError):
            job_prompts(bad, 11)
    seen = {}
    for rank in range(2):
        for batch in rank_batches(11, 4, rank, 2):
            for i in batch:
                assert i not in seen
                seen[i] = job_prompts(table, 11)[i]
    assert seen == {i: table[i] for i in range(11)}


def test_job_refuses_bad_arguments_before_it_asks_for_a_gpu():
    """a prompt or scale sequence of the wrong length and a malformed interval are ``ValueError``s of the job itself"""
    from naturaldiffusion_amd import SD3NaturalInference as S
    for kw in (dict(prompts=["a", "b", "c", "d"]), dict(prompts=["a"] * 6), dict(cfg_scale=[7.0] * 4), dict(cfg_scale=[7.0] * 6),
               dict(guidance_interval=(0.8, 0.3)), dict(guidance_interval=(0.3,)), dict(guidance_interval=(0.1, 0.2, 0.3))):
        with pytest.raises(ValueError):
            S.sd_generate_sharded(None, 5, 2, **kw)
    # the reference's one-batch job takes none of them
    for kw in (dict(prompts="a dog"), dict(negative_prompt="blurry"), dict(cfg_scale=[7.0] * 4), dict(cfg_scale=5.0), dict(guidance_interval=(0.3, 0.8))):
        with pytest.raises(ValueError):
            S.sd_natural_inference_tx(pipe=object(), decode=False, **kw)
