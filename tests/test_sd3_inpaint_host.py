"""Host-side checks of SD3 latent-space inpainting: the flow schedule of the known latents (``sampler.sd_known_schedule``), the argument
preparation of the job (``SD3NaturalInference.sd_prepare_known``: pixel-mask reduction, channel broadcast, every refusal) and the entry point's refusal
without ``sample_count``.  No GPU: everything here runs before the first launch."""
import numpy as np
import pytest
import torch

SHAPE = (16, 16, 16)
PER = 16 * 16 * 16


def test_schedule_triples_and_columns():
    from oracle import ni_oracle as O
    from naturaldiffusion_amd.sampler import KNOWN_COLUMN0, sd_known_schedule
    _, sigmas = O.sd3_sigma_schedule(28)
    sig32 = sigmas.to(torch.float32)
    sig = [float(s.to(torch.float16)) for s in sig32]
    oms = [float((1 - s).to(torch.float16)) for s in sig32]
    fresh, same = sd_known_schedule(sig, oms, "fresh"), sd_known_schedule(sig, oms, "same")
    assert len(fresh) == len(same) == 29 and KNOWN_COLUMN0 == 2 ** 31                  # N + 1 levels: the first input's, then one per step
    for j in range(29):
        assert fresh[j] == (sig[j], oms[j], 2 ** 31 + j) and same[j] == (sig[j], oms[j], 0)
        assert all(isinstance(v, float) for v in fresh[j][:2]) and isinstance(fresh[j][2], int)
        assert np.float16(fresh[j][0]) == np.float32(fresh[j][0])                      # the fp16-rounded values the step multiplies by
    assert fresh[0][:2] == (1.0, 0.0) and fresh[28][:2] == (0.0, 1.0)                  # pure noise first, the known latents themselves last
    assert sd_known_schedule(sig, oms) == fresh                                        # "fresh" is the default
    with pytest.raises(ValueError):
        sd_known_schedule(sig, oms, "mean")
    with pytest.raises(ValueError):
        sd_known_schedule(sig, oms[:-1])


def test_pixel_mask_is_reduced_to_cells_and_broadcast_over_the_channels():
    from naturaldiffusion_amd.SD3NaturalInference import sd_prepare_known
    from naturaldiffusion_amd.ValidateNaturalInference import latent_mask
    gen = torch.Generator().manual_seed(0)
    known = torch.randn(5, *SHAPE, generator=gen)
    px = torch.ones(1, 128, 128, dtype=torch.bool)
    px[0, :, 64:] = False                                                              # the right half is unknown
    px[0, 17, 3] = False                                                               # and one pixel of cell (2, 0)
    for erode in (0, 1, 2):
        got = sd_prepare_known(known, None, px, 5, SHAPE, "fresh", erode)
        cells = latent_mask(px, erode)
        assert got["mask"].dtype == torch.uint8 and tuple(got["mask"].shape) == (1, PER) and got["mask"].is_contiguous()
        assert torch.equal(got["mask"].view(1, 16, 16, 16), cells[:, None].expand(-1, 16, -1, -1))
        assert int(cells[0, :, 8 - erode:].sum()) == 0 and int(cells[0, 2, 0]) == 0 and int(cells[0, 8, 0]) == 1
    # the default erosion is one ring
    assert torch.equal(sd_prepare_known(known, None, px, 5, SHAPE)["mask"], sd_prepare_known(known, None, px, 5, SHAPE, "fresh", 1)["mask"])
    # a cell mask goes to every channel, a latent-element mask is taken as it is (non-zero = known)
    cell = torch.zeros(5, 16, 16, dtype=torch.uint8)
    cell[:, :, :5] = 7
    got = sd_prepare_known(known, None, cell, 5, SHAPE)
    assert tuple(got["mask"].shape) == (5, PER) and torch.equal(got["mask"].view(5, 16, 16, 16), (cell != 0).to(torch.uint8)[:, None].expand(-1, 16, -1, -1))
    elem = torch.randint(0, 2, (1, *SHAPE), generator=gen).bool()
    got = sd_prepare_known(known[:1], None, elem, 5, SHAPE, "same")
    assert torch.equal(got["mask"].view(1, *SHAPE), elem.to(torch.uint8))
    # the latents become the fp16 rows the step takes
    assert got["latents"].dtype == torch.float16 and torch.equal(got["latents"], known[:1].half().reshape(1, PER)) and "images" not in got
    # images are kept for the encoder
    img = torch.zeros(1, 128, 128, 3, dtype=torch.uint8)
    got = sd_prepare_known(None, img, px, 5, SHAPE)
    assert got["images"] is not None and "latents" not in got
    assert sd_prepare_known(None, torch.zeros(5, 3, 128, 128), px, 5, SHAPE)["images"].shape[0] == 5
    # none of the arguments: inpainting is off
    assert sd_prepare_known(None, None, None, 5, SHAPE) is None and sd_prepare_known(None, None, None, None, SHAPE) is None


def test_prepare_refusals():
    from naturaldiffusion_amd.SD3NaturalInference import sd_prepare_known
    known, img = torch.zeros(5, *SHAPE), torch.zeros(5, 128, 128, 3, dtype=torch.uint8)
    cell, px = torch.ones(1, 16, 16, dtype=torch.uint8), torch.ones(1, 128, 128, dtype=torch.uint8)
    bad = [dict(known_latents=known, known_images=img, mask=cell),                     # both known forms
           dict(known_latents=known, known_images=None, mask=None),                    # no mask
           dict(known_latents=None, known_images=None, mask=cell),                     # a mask alone
           dict(known_latents=known[:3], known_images=None, mask=cell),                # wrong counts: neither 1 nor sample_count
           dict(known_latents=known, known_images=None, mask=cell.expand(4, -1, -1)),
           dict(known_latents=None, known_images=img[:2], mask=px),
           dict(known_latents=known[:, :4], known_images=None, mask=cell),             # not the latent shape
           dict(known_latents=known.long(), known_images=None, mask=cell),
           dict(known_latents=known, known_images=None, mask=cell.float()),
           dict(known_latents=known, known_images=None, mask=torch.ones(1, 64, 64, dtype=torch.uint8)),   # neither cells nor pixels
           dict(known_latents=None, known_images=torch.zeros(1, 64, 64, 3, dtype=torch.uint8), mask=cell),
           dict(known_latents=None, known_images=torch.zeros(1, 128, 128, 3), mask=cell),                  # fp32 images are NCHW
           dict(known_latents=known, known_images=None, mask=cell, renoise="mean"),    # a bad renoise
           dict(known_latents=known, known_images=None, mask=px, mask_erode=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            sd_prepare_known(kw["known_latents"], kw["known_images"], kw["mask"], 5, SHAPE, kw.get("renoise", "fresh"), kw.get("mask_erode", 1))
    with pytest.raises(ValueError):                                                    # a bad renoise is refused without the other arguments too
        sd_prepare_known(None, None, None, 5, SHAPE, "mean")
    with pytest.raises(ValueError):                                                    # the arguments without sample_count
        sd_prepare_known(known, None, cell, None, SHAPE)
    # known_images beyond the encoder engine: 1024 x 1024 pixels is latent side 128
    big = (16, 128, 128)
    with pytest.raises(ValueError, match="known_latents"):
        sd_prepare_known(None, torch.zeros(1, 1024, 1024, 3, dtype=torch.uint8), torch.ones(1, 128, 128, dtype=torch.uint8), 5, big)
    got = sd_prepare_known(torch.zeros(1, *big), None, torch.ones(1, 128, 128, dtype=torch.uint8), 5, big)       # known_latents at that size are fine
    assert tuple(got["latents"].shape) == (1, 16 * 128 * 128)
    assert sd_prepare_known(None, torch.zeros(1, 512, 512, 3, dtype=torch.uint8), torch.ones(1, 64, 64, dtype=torch.uint8), 5, (16, 64, 64)) is not None


def test_entry_point_refuses_the_arguments_without_sample_count():
    from naturaldiffusion_amd import SD3NaturalInference as S
    known, cell = torch.zeros(1, *SHAPE), torch.ones(1, 16, 16, dtype=torch.uint8)
    for kw in (dict(known_latents=known, mask=cell), dict(known_images=torch.zeros(1, 128, 128, 3, dtype=torch.uint8), mask=cell), dict(mask=cell),
               dict(renoise="same"), dict(mask_erode=2)):
        with pytest.raises(ValueError, match="sample_count"):
            S.sd_natural_inference_tx(pipe=object(), decode=False, **kw)
    with pytest.raises(ValueError):                                                    # and the job itself refuses before it touches the pipe or a GPU
        S.sd_generate_sharded(object(), 5, 2, latent_shape=SHAPE, known_latents=known, known_images=torch.zeros(1, 128, 128, 3, dtype=torch.uint8), mask=cell)
    with pytest.raises(ValueError):
        S.sd_generate_sharded(object(), 5, 2, latent_shape=SHAPE, renoise="other")
