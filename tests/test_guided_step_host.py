"""Host-side checks of per-image guidance: the argument errors of natinf_step_f32prod_noise_guided that are decided before
any device is touched (include/natinf.h; dummy pointers are never dereferenced by the argument check, and there is no GPU
here), and the pure planning functions of the DiT job (``ValidateNaturalInference.job_scales`` / ``guidance_plan``)."""
import numpy as np
import pytest

from naturaldiffusion_amd.coeff import load_coeff_npz

D = 4096                                                      # a non-NULL dummy pointer
ARGS = ("z", "cond", "uncond", "cfg_image", "uncond_slot", "n_uncond", "sample_elems", "eps_sample_stride", "hist_x0", "noise", "z_next",
        "idx_c", "val_c", "n_c", "c_diag", "idx_b", "val_b", "n_b", "k", "c1", "c2", "seed", "image_index", "first_index", "index_stride",
        "E", "stream")
GOOD = dict(z=D, cond=D, uncond=D, cfg_image=D, uncond_slot=D, n_uncond=2, sample_elems=8, eps_sample_stride=8, hist_x0=D, noise=D, z_next=D,
            idx_c=D, val_c=D, n_c=1, c_diag=1.0, idx_b=D, val_b=D, n_b=2, k=1, c1=1.0, c2=0.5, seed=7, image_index=None, first_index=0,
            index_stride=1, E=16, stream=None)


def call(**kw):
    from naturaldiffusion_amd._lib import lib
    a = {**GOOD, **kw}
    return lib.natinf_step_f32prod_noise_guided(*[a[name] for name in ARGS])


def test_guided_entry_argument_errors():
    """every refusal is NATINF_EINVAL (-1) before a device is asked for anything"""
    for name in ("z", "cond", "hist_x0", "z_next"):
        assert call(**{name: None}) == -1, name
    assert call(cfg_image=None) == -1 and call(uncond_slot=None) == -1                  # the two per-image arrays
    assert call(n_uncond=-1) == -1                                                       # a negative row count
    assert call(n_uncond=1, uncond=None) == -1 and call(n_uncond=2, uncond=None) == -1   # rows announced, none given
    # and every refusal of natinf_step_f32prod_noise
    assert call(E=14) == -1 and call(E=0) == -1 and call(E=-16) == -1                    # E % 4, E > 0
    assert call(sample_elems=6) == -1 and call(sample_elems=0) == -1                     # sample_elems % 4
    assert call(E=12, sample_elems=8) == -1                                              # E % sample_elems
    assert call(E=4 * 2 ** 32, sample_elems=4 * 2 ** 32, eps_sample_stride=4 * 2 ** 32) == -1   # the quad does not fit counter word 2
    assert call(eps_sample_stride=4) == -1 and call(eps_sample_stride=10) == -1          # stride below the sample, stride % 4
    assert call(k=-1) == -1
    assert call(n_b=-1) == -1 and call(idx_b=None) == -1 and call(val_b=None) == -1      # terms_ok of the noise row
    assert call(n_c=-1) == -1 and call(idx_c=None) == -1 and call(val_c=None) == -1      # terms_ok of the signal row
    assert call(n_b=4, k=1) == -1 and call(n_b=3, k=0) == -1                             # more terms than columns 0..k+1


@pytest.fixture(scope="module")
def node(repo_root):
    return load_coeff_npz(repo_root / "results/ddpm/ddpm_024.npz")[2]


def test_plan_without_interval_guides_every_step(node):
    from naturaldiffusion_amd.ValidateNaturalInference import guidance_plan, job_scales
    for n in (1, 4, 7):
        guided, slots, scales = guidance_plan(node, 24, job_scales(4.0, n), None)
        assert guided == [True] * 24 and slots == list(range(n)) and scales == [4.0] * n


def test_plan_interval_is_inclusive_on_the_timestep_grid(node):
    from naturaldiffusion_amd.ValidateNaturalInference import guidance_plan
    ts = [int(node[kk, 0]) for kk in range(24)]
    assert len(set(ts)) == 24 and ts == sorted(ts, reverse=True) and ts[-1] >= 0, "the job feeds 24 distinct descending timesteps"
    # an interval between two neighbouring grid points holds no timestep: nothing is guided
    gap = next((b + 1, a - 1) for a, b in zip(ts, ts[1:]) if a - b >= 2)
    assert guidance_plan(node, 24, [4.0] * 3, gap)[0] == [False] * 24
    assert guidance_plan(node, 24, [4.0] * 3, (ts[0] + 1, ts[0] + 500))[0] == [False] * 24
    # some: exactly the kk whose timestep lies in it
    lo, hi = 200, 800
    want = [lo <= t <= hi for t in ts]
    assert 0 < sum(want) < 24
    guided, slots, _ = guidance_plan(node, 24, [4.0] * 3, (lo, hi))
    assert guided == want and slots == [0, 1, 2]
    # a grid point as either end is inside; one past it is outside
    a, b = ts[17], ts[5]                                       # a < b
    assert guidance_plan(node, 24, [2.0], (a, b))[0] == [5 <= kk <= 17 for kk in range(24)]
    assert guidance_plan(node, 24, [2.0], (a + 1, b))[0] == [5 <= kk <= 16 for kk in range(24)]
    assert guidance_plan(node, 24, [2.0], (a, b - 1))[0] == [6 <= kk <= 17 for kk in range(24)]
    assert guidance_plan(node, 24, [2.0], (a, a))[0] == [kk == 17 for kk in range(24)]
    # an interval over everything is the plan without one
    assert guidance_plan(node, 24, [2.0], (0, 999)) == guidance_plan(node, 24, [2.0], None)


def test_plan_compacts_the_guided_images(node):
    from naturaldiffusion_amd.ValidateNaturalInference import guidance_plan
    guided, slots, scales = guidance_plan(node, 24, [4, 1, 2.5, 1, 1.5], None)
    assert slots == [0, -1, 1, -1, 2] and scales == [4.0, 1.0, 2.5, 1.0, 1.5] and guided == [True] * 24
    # every scale 1: no image has a slot, so no step runs an unconditional sample, interval or not
    for interval in (None, (0, 999)):
        guided, slots, _ = guidance_plan(node, 24, [1.0, 1, 1.0], interval)
        assert slots == [-1, -1, -1] and guided == [False] * 24
    # the scale is the fp32 value the kernel multiplies by
    assert guidance_plan(node, 24, [0.1], None)[2] == [float(np.float32(0.1))]


def test_job_scales_follow_the_global_index():
    from naturaldiffusion_amd.ValidateNaturalInference import job_batches, job_scales
    assert job_scales(4.0, 3) == [4.0, 4.0, 4.0] and job_scales(2, 2) == [2.0, 2.0] and job_scales(4.0, 0) == []
    table = [1.0 + 0.25 * (i % 7) for i in range(23)]
    assert job_scales(table, 23) == table and job_scales(np.asarray(table), 23) == table
    for bad in (table[:22], table + [1.0], []):
        with pytest.raises(ValueError):
            job_scales(bad, 23)
    # sharding: image i gets table[i] on whichever rank owns it, whatever the batch size
    for batch_size in (1, 3, 4, 32):
        seen = {}
        for rank in range(2):
            for indices, _ in job_batches(23, batch_size, rank, 2):
                scales = job_scales(table, 23)
                for i in indices:
                    assert i not in seen
                    seen[i] = scales[i]
        assert seen == {i: table[i] for i in range(23)}
