"""Posterior statistics on the GPU (include/natinf_posterior.h; AnalyzeWeightedSumDegradation.posterior_stats / get_statistics) against
tests/posterior_oracle.py: the samples bit for bit, the two row statistics no further from an fp64 evaluation than the reference's own fp32
statements are, the edges of the softmax, the flow form and the sharded job.

Accuracy figures measured on the MI355X (rms error over the competing rows relative to the reference's, p_diag / p_max; the bound is 1.0):
see profiles/posterior/accuracy.txt, written by this module's accuracy tests when NATINF_POSTERIOR_ACCURACY_OUT names a file."""
import os

import numpy as np
import pytest
import torch

import posterior_oracle as O
from naturaldiffusion_amd import AnalyzeWeightedSumDegradation as A

pytestmark = pytest.mark.gpu

# the last shape is this file's own: d at its limit and few tiles, so a block runs 32 K tiles and adds its fp32 accumulators into the fp64 ones four times
SHAPES = [(1, 64), (37, 192), (129, 1024), (257, 4096), (70, 16384), (5, 65536)]
SEED = 2            # of the competing-rows recipe: the share of rows with p_max in (0.05, 0.95) is 0.80 / 0.31 / 1.0 at the three accuracy shapes (vp, t = 200)

_cache = {}


def _case(form, t, n, d):
    """feats (bf16), the reference's noise stream, the reference's samples, and the exact / reference statistics: computed once"""
    key = (form, t, n, d)
    if key not in _cache:
        a, b, sigma = A.level_scalars(form, t)
        feats = O.competing_feats(n, d, b, SEED)
        noise = torch.randn(n, d, generator=torch.Generator().manual_seed(100 + SEED))
        samples = O.add_noise(feats.float(), noise, a, b)
        _cache[key] = dict(a=a, b=b, sigma=sigma, feats=feats, noise=noise, samples=samples, stats={})
    return _cache[key]


def _oracle_stats(case):
    if not case["stats"]:
        case["stats"]["exact"] = O.exact_stats(case["samples"], case["feats"].float(), case["sigma"])
        case["stats"]["reference"] = O.reference_stats(case["samples"], case["feats"].float(), case["sigma"])
    return case["stats"]["exact"], case["stats"]["reference"]


def _philox(seed, index, d):
    from naturaldiffusion_amd import _lib
    out = torch.empty(index.numel(), d, dtype=torch.float32, device="cuda")
    idx = index.cuda().contiguous()
    _lib.check(_lib.lib.natinf_randn_philox_f32(_lib.ptr(out), index.numel(), d, _lib.ptr(idx), 0, 1, seed, _lib.stream_ptr()), "natinf_randn_philox_f32")
    return out.cpu()


def _check_samples(form, t, n, d):
    c = _case(form, t, n, d)
    got = A.PosteriorSamples(c["feats"], c["a"], c["b"], noise=c["noise"]).samples()
    assert torch.equal(got, c["samples"]), f"{(got != c['samples']).sum().item()} of {got.numel()} samples differ from torch's fp32 statement"
    # Philox, with an index that is neither contiguous nor ordered
    index = ((torch.arange(2 * n, dtype=torch.int64) * 7919 + 3) % 1000003 + (5 << 20))[::2]
    assert n == 1 or not index.is_contiguous()
    eps = _philox(11, index, d)
    got = A.PosteriorSamples(c["feats"], c["a"], c["b"], seed=11, index=index).samples()
    assert torch.equal(got, O.add_noise(c["feats"].float(), eps, c["a"], c["b"]))
    assert float(eps.std()) > 0.5 and (n == 1 or not torch.equal(eps[0], eps[-1]))


def _check_accuracy(form, t, n, d):
    c = _case(form, t, n, d)
    (ed, em), (rd, rm) = _oracle_stats(c)
    sel = (em > 0.05) & (em < 0.95)
    assert float(sel.double().mean()) >= 0.25, "the input does not make rows compete: pick another seed"
    pd, pm = A.posterior_stats(c["feats"], c["a"], c["b"], c["sigma"], noise=c["noise"])
    ratios = (O.rms((pd - ed)[sel]) / O.rms((rd - ed)[sel]), O.rms((pm - em)[sel]) / O.rms((rm - em)[sel]))
    line = (f"{form} t={t} (n, d) = ({n}, {d}): rms error over {int(sel.sum())} competing rows relative to the reference's: p_diag {ratios[0]:.3f} "
            f"(reference {O.rms((rd - ed)[sel]):.2e}), p_max {ratios[1]:.3f} (reference {O.rms((rm - em)[sel]):.2e})")
    print(line)
    if os.environ.get("NATINF_POSTERIOR_ACCURACY_OUT"):
        with open(os.environ["NATINF_POSTERIOR_ACCURACY_OUT"], "a") as fh:
            fh.write(line + "\n")
    assert torch.isfinite(pd).all() and torch.isfinite(pm).all() and (pd >= 0).all() and (pm <= 1).all() and (pm >= pd).all()
    assert ratios[0] <= 1.0 and ratios[1] <= 1.0, line


@pytest.mark.parametrize("n,d", SHAPES)
def test_samples_bit_for_bit(n, d):
    _check_samples("vp", 200, n, d)


# beside the three shapes the contract names, the two ragged ones: their rows compete too (share 1.0), so the same bound applies
@pytest.mark.parametrize("n,d", [(129, 1024), (257, 4096), (70, 16384), (37, 192), (5, 65536)])
def test_accuracy_no_worse_than_the_reference(n, d):
    _check_accuracy("vp", 200, n, d)


def test_edges():
    n, d = 37, 192
    c = _case("vp", 200, n, d)
    feats, noise = c["feats"].clone(), c["noise"].clone()
    feats[20], noise[20] = feats[3], noise[3]                                     # an exact tie: rows 3 and 20 are one point
    # with little noise a row's own image is its nearest, so the pair shares the row maximum (at the level's own noise another row may well be nearer)
    pd, pm = A.posterior_stats(feats, 1.0, 1e-3, c["sigma"], noise=noise)
    assert pd[3] == pm[3] == pd[20] == pm[20] and 0 < pd[3] <= 0.5
    assert (pd == pm).all()
    smp = A.PosteriorSamples(feats, c["a"], c["b"], noise=noise)
    pd, pm = smp.stats(c["sigma"])
    assert pd[3] == pd[20] and pm[3] == pm[20]                                      # the tie itself holds at any noise
    # sigma -> 0 with little noise: every row's own image takes all the mass, exactly
    pd0, pm0 = A.posterior_stats(feats[:20], 1.0, 1e-3, 1e-3, noise=noise[:20])
    assert (pd0 == 1.0).all() and (pm0 == 1.0).all()
    # sigma -> infinity: uniform
    pd1, pm1 = smp.stats(1e6)
    assert float((pd1 - 1 / n).abs().max()) <= 1e-6 and float((pm1 - 1 / n).abs().max()) <= 1e-6
    for sigma in (1e-3, 1e-30, 0.05, 1e6, 1e200):
        p, q = smp.stats(sigma)
        assert torch.isfinite(p).all() and torch.isfinite(q).all() and (p >= 0).all() and (q <= 1).all() and (q >= p).all(), sigma
    one = _case("vp", 200, 1, 64)
    p, q = A.posterior_stats(one["feats"], one["a"], one["b"], one["sigma"], noise=one["noise"])
    assert p.tolist() == [1.0] and q.tolist() == [1.0]


@pytest.mark.parametrize("n,d", [(37, 192), (257, 4096)])
def test_flow_form(n, d):
    _check_samples("flow", 300, n, d)
    _check_accuracy("flow", 300, n, d)


def test_job_level():
    sizes, d, ts = [5, 37, 130], 192, (200, 600)
    b = A.level_scalars("vp", 200)[1]
    # twice the accuracy tests' spread: at t = 200 a few rows of every class (2, 4 and 3) hold more than 0.9 of their posterior, none at t = 600
    classes = [O.competing_feats(n, d, 2 * b, 10 + i) for i, n in enumerate(sizes)]
    whole = A.get_statistics(classes, form="vp", ts=ts, seed=5)
    merged = A.merge_statistics([A.get_statistics([(lambda f=f: f) for f in classes], form="vp", ts=ts, seed=5, rank=r, world=2) for r in (0, 1)])
    for t in ts:
        w, m = whole[t], merged[t]
        assert np.array_equal(w["hist_x0"], m["hist_x0"]) and np.array_equal(w["hist_xx"], m["hist_xx"])
        assert w["classes"] == m["classes"] == [0, 1, 2] and w["x0_counts"] == m["x0_counts"] and w["xx_counts"] == m["xx_counts"]
        assert w["total_count"] == m["total_count"] == sum(sizes) == w["hist_x0"].sum() == w["hist_xx"].sum()
        a, b_t, sigma = A.level_scalars("vp", t)
        for ci, f in enumerate(classes):
            index = (ci << 20) + torch.arange(sizes[ci], dtype=torch.int64)
            ed, em = O.exact_stats(O.add_noise(f.float(), _philox(5, index, d), a, b_t), f.float(), sigma)
            assert float((ed - 0.9).abs().min()) > 1e-3, "an exact p_ii lies within 1e-3 of 0.9: change the inputs"
            assert w["x0_counts"][ci] == int((ed > 0.9).sum())
            assert abs(w["xx_counts"][ci] - float(em.sum())) <= 1e-3 * sizes[ci]
