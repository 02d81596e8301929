"""Host-side checks of ``naturaldiffusion_amd.jobs``, what the three generation jobs share: the ``KnownRows`` tables (sharded gathering, the encoder
callback's chunks, the shared row), the generic ``guidance_plan`` against the DiT and SD3 wrappers, and the reduction of a mask to one byte per
latent element.  No GPU: ``KnownRows`` is given the CPU as its device."""
import numpy as np
import pytest
import torch

from naturaldiffusion_amd import jobs
from naturaldiffusion_amd.shard import rank_batches

WORLD, BATCH, E = 2, 3, 8


def table(k):
    return torch.arange(k * E, dtype=torch.float32).reshape(k, E) * 0.5 + 1.0


def test_jobs_imports_nothing_of_the_package():
    """host code only: numpy and torch, so importing it cannot load the library or ask for a GPU"""
    import ast
    tree = ast.parse(open(jobs.__file__).read())
    names = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    froms = {(n.level, (n.module or "").split(".")[0]) for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert names == {"numpy", "torch"} and froms == {(0, "__future__")}


@pytest.mark.parametrize("k", [1, 7])
def test_known_rows_hand_a_batch_the_rows_of_its_global_indices(k):
    """tables given by global index (K = 7) or as one shared row (K = 1), rank-sharded batches of 3 with a ragged last one"""
    full, mask = table(k), (torch.arange(k * E).reshape(k, E) % 3 == 0).to(torch.uint8)
    for rank in range(WORLD):
        batches = list(rank_batches(7, BATCH, rank, WORLD))
        assert [len(b) for b in batches] == ([3, 1] if rank == 0 else [3])                 # rank 0: 0 2 4 | 6, rank 1: 1 3 5
        rows = jobs.KnownRows("cpu", known=full, mask=mask)
        for b in batches:
            got = rows.batch(b)
            assert sorted(got) == ["known", "mask"] and got["known"].dim() == 1 and got["mask"].dtype == torch.uint8
            want = torch.tensor([0] if k == 1 else b)
            assert torch.equal(got["known"], full[want].reshape(-1)) and torch.equal(got["mask"], mask[want].reshape(-1))
        if k == 1:                                                                         # the one row is made once and handed to every batch
            assert rows.batch(batches[0])["known"] is rows.batch(batches[-1])["known"]


@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("max_batch", [1, 2, 5])
def test_known_rows_encode_asks_for_each_needed_row_once(k, max_batch):
    """a table that holds only this rank's encoded rows, in the rank's order, is read back through the rows-of-this-rank index"""
    source = table(k)
    encoded = lambda t: t * 2.0 + 3.0
    for rank in range(WORLD):
        batches, seen = list(rank_batches(7, BATCH, rank, WORLD)), []

        def encode_chunk(chunk, idx):
            assert 0 < len(idx) <= max_batch and torch.equal(chunk, source[torch.tensor(idx)])
            seen.extend(idx)
            return encoded(chunk)
        rows = jobs.KnownRows("cpu", mask=torch.ones(1, E, dtype=torch.uint8))
        rows.encode("known", source, batches, encode_chunk, max_batch)
        mine = [i for b in batches for i in b]
        assert seen == ([0] if k == 1 else mine), "every needed row exactly once, in the rank's order"
        assert rows.tables["known"].shape[0] == (1 if k == 1 else len(mine))               # this rank's rows only
        for b in batches:
            want = torch.tensor([0] if k == 1 else b)
            assert torch.equal(rows.batch(b)["known"], encoded(source)[want].reshape(-1))
        assert seen == ([0] if k == 1 else mine), "handing out batches encodes nothing again"


def test_known_rows_of_a_rank_without_batches_encode_nothing():
    rows = jobs.KnownRows("cpu")
    rows.encode("known", table(7), [], lambda chunk, idx: pytest.fail("nothing to encode"), 4)
    assert "known" not in rows.tables


def plan_by_hand(levels, scales, interval):
    """the rule restated image by image and step by step"""
    scales = [float(np.float32(v)) for v in scales]
    slots = []
    for v in scales:
        slots.append(-1 if v == 1.0 else sum(s >= 0 for s in slots))
    guided = [any(s >= 0 for s in slots) and (interval is None or interval[0] <= lv <= interval[1]) for lv in levels]
    return guided, slots, scales


SCALES = {"all one": [1.0, 1, 1.0], "mixed": [4, 1, 2.5, 1.0, 0.1], "all guided": [7.0] * 4}


@pytest.mark.parametrize("name", list(SCALES))
def test_generic_plan_reproduces_both_wrappers(repo_root, name):
    from naturaldiffusion_amd.coeff import load_coeff_npz
    from naturaldiffusion_amd.SD3NaturalInference import sd_guidance_plan
    from naturaldiffusion_amd.ValidateNaturalInference import guidance_plan
    from oracle import ni_oracle as O
    scales = SCALES[name]
    node = load_coeff_npz(repo_root / "results/ddpm/ddpm_024.npz")[2]
    ts = [int(node[kk, 0]) for kk in range(24)]
    for interval in (None, (ts[17], ts[5]), (ts[0] + 1, ts[0] + 500)):                     # no interval, steps 5..17, an interval that excludes every step
        got = jobs.guidance_plan(ts, 24, scales, interval)
        assert got == plan_by_hand(ts, scales, interval) == guidance_plan(node, 24, scales, interval)
        if interval == (ts[0] + 1, ts[0] + 500) or name == "all one":
            assert got[0] == [False] * 24
    sigmas = O.sd3_sigma_schedule(28)[1]
    sg = [float(sigmas[kk]) for kk in range(28)]
    for interval in (None, (0.3, 0.8), (1.5, 2.0)):
        got = jobs.guidance_plan(sg, 28, scales, interval)
        assert got == plan_by_hand(sg, scales, interval) == sd_guidance_plan(sigmas, 28, scales, interval)
        if interval == (1.5, 2.0) or name == "all one":
            assert got[0] == [False] * 28
    if name == "mixed":
        assert got[1] == [0, -1, 1, -1, 2] and got[2][4] == float(np.float32(0.1))


def test_interval_check_words_the_refusal_of_its_caller():
    jobs.check_interval(None)
    jobs.check_interval((3, 3), int, "t_lo", "t_hi")
    with pytest.raises(ValueError, match=r"\(t_lo, t_hi\) with t_lo <= t_hi"):
        jobs.check_interval((4, 3), int, "t_lo", "t_hi")
    with pytest.raises(ValueError, match=r"\(s_lo, s_hi\) with s_lo <= s_hi"):
        jobs.check_interval((0.5, 0.25))
    with pytest.raises(ValueError, match="guidance_interval"):
        jobs.check_interval((0.1, 0.2, 0.3))


def test_scalar_scale_predicate():
    for v in (4, 4.0, np.float32(4), np.int64(4)):
        assert jobs.is_scalar_scale(v)
    for v in ([4.0], (4.0,), np.asarray([4.0]), torch.tensor([4.0])):
        assert not jobs.is_scalar_scale(v)


def test_mask_forms_of_one_mask_give_one_table():
    """a 2-channel latent of side 2: the element, cell and pixel (``mask_erode=0``) forms of the same mask"""
    ch, S, K = 2, 2, 3
    cells = torch.tensor([[[1, 0], [0, 1]], [[0, 0], [1, 1]], [[1, 1], [1, 0]]], dtype=torch.uint8)
    element = cells[:, None].expand(-1, ch, -1, -1).contiguous()
    pixel = torch.from_numpy(np.kron(cells.numpy(), np.ones((8, 8), np.uint8)))
    want = element.reshape(K, ch * S * S)
    for m in (element, cells, pixel, cells.bool(), pixel * 255):
        got = jobs.mask_table(jobs.host_mask(m), ch, S, K, 0)
        assert got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got, want)
    assert torch.equal(jobs.mask_table(cells[:1], ch, S, K, 0), want[:1])                  # one shared row
    # erosion is the pixel form's alone: one ring takes every cell of this mask that has an unknown neighbour
    assert int(jobs.mask_table(pixel, ch, S, K, 1).sum()) == 0 and torch.equal(jobs.mask_table(cells, ch, S, K, 1), want)
    # a form the caller does not accept, or no form at all: None, the caller words the refusal
    assert jobs.mask_table(pixel, ch, S, K, 0, forms=("element", "cell")) is None
    assert jobs.mask_table(cells, ch, S, K, 0, forms=("pixel",)) is None
    assert jobs.mask_table(torch.ones(K, 3, 3, dtype=torch.uint8), ch, S, K, 0) is None
    with pytest.raises(ValueError, match="bool or uint8"):
        jobs.host_mask(torch.ones(K, S, S))


@pytest.mark.parametrize("rows", [2, 4])
def test_row_count_rule(rows):
    """K is 1 or sample_count (3)"""
    with pytest.raises(ValueError, match=rf"mask must hold 1 row \(shared\) or sample_count \(3\) rows, not {rows}"):
        jobs.mask_table(torch.ones(rows, 2, 2, dtype=torch.uint8), 2, 2, 3, 0)
    with pytest.raises(ValueError, match=rf"known must hold 1 row \(shared\) or sample_count \(3\) rows, not {rows}"):
        jobs.check_row_count("known", torch.zeros(rows, 8), 3)
    jobs.check_row_count("known", torch.zeros(1, 8), 3)
    jobs.check_row_count("known", torch.zeros(3, 8), 3)


def test_either_or_rule_of_the_inpainting_arguments():
    t = torch.zeros(1)
    assert jobs.inpainting_on(None, None, None) is False
    assert jobs.inpainting_on(t, None, t) is True and jobs.inpainting_on(None, t, t) is True
    for args, word in (((t, t, t), "not both"), ((t, None, None), "needs mask="), ((None, t, None), "needs mask="), ((None, None, t), "mask= needs")):
        with pytest.raises(ValueError, match=word):
            jobs.inpainting_on(*args)
