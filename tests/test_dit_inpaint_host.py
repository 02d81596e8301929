"""Host-side checks of latent-space inpainting on the DiT path: the argument errors of natinf_step_f32prod_inpaint that are decided before any
device is touched (include/natinf.h; dummy pointers are never dereferenced by the argument check, and there is no GPU here), the pixel-to-cell
mask reduction ``ValidateNaturalInference.latent_mask`` against a brute-force window loop, the argument errors of ``generate_sharded`` that come
before a model is needed, and the levels ``known_schedule`` reads off the DiT node tables."""
import numpy as np
import pytest
import torch

from naturaldiffusion_amd.coeff import load_coeff_npz

D = 4096                                                      # a non-NULL dummy pointer, 4-byte aligned
ARGS = ("z", "cond", "uncond", "cfg_image", "uncond_slot", "n_uncond", "sample_elems", "eps_sample_stride", "hist_x0", "noise", "z_next",
        "idx_c", "val_c", "n_c", "c_diag", "idx_b", "val_b", "n_b", "k", "c1", "c2", "seed", "image_index", "first_index", "index_stride",
        "E", "known", "mask", "known_image_stride", "mask_image_stride", "known_alpha", "known_std", "known_column", "stream")
GOOD = dict(z=D, cond=D, uncond=D, cfg_image=D, uncond_slot=D, n_uncond=2, sample_elems=8, eps_sample_stride=8, hist_x0=D, noise=D, z_next=D,
            idx_c=D, val_c=D, n_c=1, c_diag=1.0, idx_b=D, val_b=D, n_b=2, k=1, c1=1.0, c2=0.5, seed=7, image_index=None, first_index=0,
            index_stride=1, E=16, known=D, mask=D, known_image_stride=8, mask_image_stride=0, known_alpha=0.5, known_std=0.5,
            known_column=2 ** 31 + 2, stream=None)


def call(**kw):
    from naturaldiffusion_amd._lib import lib
    a = {**GOOD, **kw}
    return lib.natinf_step_f32prod_inpaint(*[a[name] for name in ARGS])


def test_inpaint_entry_argument_errors():
    """every refusal is NATINF_EINVAL (-1) before a device is asked for anything: the pure checks come before the two read-backs"""
    # what the blend adds, with elems_per_image = sample_elems
    assert call(known=None) == -1 and call(mask=None) == -1
    for bad in (4, 16, -8, 12):                                                          # a stride is 0 or sample_elems (8)
        assert call(known_image_stride=bad) == -1, bad
        assert call(mask_image_stride=bad) == -1, bad
    for off in (1, 2, 3):
        assert call(mask=D + off) == -1, off                                             # the mask is read as 32-bit words
    assert call(known_column=2 ** 31 - 1) == -1 and call(known_column=0) == -1 and call(known_column=2) == -1
    # every refusal of natinf_step_f32prod_noise_guided
    for name in ("z", "cond", "hist_x0", "z_next"):
        assert call(**{name: None}) == -1, name
    assert call(cfg_image=None) == -1 and call(uncond_slot=None) == -1
    assert call(n_uncond=-1) == -1
    assert call(n_uncond=1, uncond=None) == -1 and call(n_uncond=2, uncond=None) == -1
    # ... which include every refusal of natinf_step_f32prod_noise
    assert call(E=14) == -1 and call(E=0) == -1 and call(E=-16) == -1
    assert call(sample_elems=6) == -1 and call(sample_elems=0) == -1
    assert call(E=12, sample_elems=8) == -1
    big = 4 * 2 ** 32
    assert call(E=big, sample_elems=big, eps_sample_stride=big, known_image_stride=big) == -1   # the quad does not fit counter word 2
    assert call(eps_sample_stride=4) == -1 and call(eps_sample_stride=10) == -1
    assert call(k=-1) == -1
    assert call(n_b=-1) == -1 and call(idx_b=None) == -1 and call(val_b=None) == -1
    assert call(n_c=-1) == -1 and call(idx_c=None) == -1 and call(val_c=None) == -1
    assert call(n_b=4, k=1) == -1 and call(n_b=3, k=0) == -1


def test_the_entry_has_a_signature_and_the_abi_version_stays():
    from naturaldiffusion_amd import _lib
    assert "natinf_step_f32prod_inpaint" in _lib.SIGNATURES
    guided, inpaint = _lib.SIGNATURES["natinf_step_f32prod_noise_guided"][1], _lib.SIGNATURES["natinf_step_f32prod_inpaint"][1]
    assert inpaint[:len(guided) - 1] == guided[:-1] and len(inpaint) == len(guided) + 7   # the guided entry's arguments up to E, then the blend's seven
    assert _lib.lib.natinf_abi_version() == 1


# ------------------------------------------------------------------------------ latent_mask
def brute_latent_mask(m, erode):
    """cell (i, j) is known iff every pixel of the (8 + 16*erode)-pixel square centred on it that lies inside the image is known"""
    K, H, W = m.shape
    out = np.zeros((K, H // 8, W // 8), np.uint8)
    for k in range(K):
        for i in range(H // 8):
            for j in range(W // 8):
                r0, r1 = max(0, 8 * (i - erode)), min(H, 8 * (i + 1 + erode))
                c0, c1 = max(0, 8 * (j - erode)), min(W, 8 * (j + 1 + erode))
                out[k, i, j] = bool((m[k, r0:r1, c0:c1] != 0).all())
    return out


@pytest.mark.parametrize("erode", [0, 1, 2])
def test_latent_mask_against_the_window_loop(erode):
    from naturaldiffusion_amd.ValidateNaturalInference import latent_mask
    rs = np.random.RandomState(erode)
    # a random mask, mostly known (so that some cells survive the erosion), as uint8 with several non-zero values
    rnd = (rs.rand(2, 64, 64) > 0.003 / (2 * erode + 1) ** 2).astype(np.uint8) * rs.choice(np.array([1, 2, 255], np.uint8), size=(2, 64, 64))
    # a rectangular hole that straddles cell borders, and its complement (a known rectangle)
    hole = np.ones((1, 64, 64), np.uint8)
    hole[0, 13:38, 20:51] = 0
    rect = 1 - hole
    for m in (rnd, hole, rect, hole.astype(bool)):
        got = latent_mask(torch.from_numpy(m), erode)
        want = brute_latent_mask(m, erode)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.numpy(), want), erode
    assert 0 < brute_latent_mask(rnd, erode).sum() < rnd.size // 64
    assert 0 < brute_latent_mask(hole, erode).sum() < 64
    # erode 0 on a cell-aligned mask is the mask itself, cell by cell
    cells = rs.rand(1, 8, 8) > 0.5
    assert np.array_equal(latent_mask(torch.from_numpy(np.kron(cells, np.ones((8, 8), bool))), 0).numpy(), cells.astype(np.uint8))
    with pytest.raises(ValueError):
        latent_mask(torch.ones(1, 60, 64, dtype=torch.uint8), erode)
    with pytest.raises(ValueError):
        latent_mask(torch.ones(1, 64, 64), erode)                                        # a float mask
    with pytest.raises(ValueError):
        latent_mask(torch.ones(1, 64, 64, dtype=torch.uint8), -1)


# ------------------------------------------------------------------------------ the job's argument errors
def test_job_argument_errors_come_before_a_model_is_needed():
    """no model, no model_path, no GPU: a ValueError, never the RuntimeError that asks for a denoiser"""
    from naturaldiffusion_amd import ValidateNaturalInference as V
    assert V.model_path is None and V.denoiser_factory is None
    S, n = 32, 3
    kl, ki = torch.zeros(n, 4, S, S), torch.zeros(n, 8 * S, 8 * S, 3, dtype=torch.uint8)
    mc, mp = torch.ones(n, S, S, dtype=torch.bool), torch.ones(1, 8 * S, 8 * S, dtype=torch.uint8)
    bad = [dict(known_latents=kl, known_images=ki, mask=mc),                             # both
           dict(known_latents=kl), dict(known_images=ki), dict(mask=mc),                 # one without the mask, the mask alone
           dict(known_latents=kl, mask=mc, known_final="sample"),
           dict(known_latents=kl[:2], mask=mc), dict(known_latents=kl, mask=mc[:2]),     # K, K' in {1, sample_count}
           dict(known_latents=kl.double(), mask=mc), dict(known_latents=kl[:, :3], mask=mc),
           dict(known_latents=kl, mask=mc.float()), dict(known_latents=kl, mask=mp),     # a pixel mask with latents
           dict(known_images=ki, mask=mc),                                               # a cell mask with images
           dict(known_images=ki[:, :, :, :2], mask=mp), dict(known_images=ki.float(), mask=mp),
           dict(known_images=ki, mask=mp, mask_erode=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            V.generate_sharded(n, None, decode=False, **kw)
    # good arguments get as far as the missing denoiser
    for kw in (dict(known_latents=kl, mask=mc), dict(known_latents=kl[:1], mask=mc[:1, None].expand(-1, 4, -1, -1)), dict(known_images=ki, mask=mp),
               dict(known_images=torch.zeros(1, 3, 8 * S, 8 * S), mask=mp)):
        with pytest.raises(RuntimeError):
            V.generate_sharded(n, None, decode=False, **kw)


def test_prepared_mask_is_one_byte_per_latent_element():
    from naturaldiffusion_amd.ValidateNaturalInference import prepare_known_latents, latent_mask, gather_rows
    S = 8
    rs = np.random.RandomState(0)
    cells = torch.from_numpy(rs.rand(3, S, S) > 0.5)
    p = prepare_known_latents(torch.zeros(1, 4, S, S), None, cells, 3)
    assert p["S"] == S and p["mask"].dtype == torch.uint8 and tuple(p["mask"].shape) == (3, 4 * S * S) and tuple(p["latents"].shape) == (1, 4 * S * S)
    assert torch.equal(p["mask"].view(3, 4, S, S), cells[:, None].expand(-1, 4, -1, -1).to(torch.uint8))
    px = torch.from_numpy(rs.rand(1, 8 * S, 8 * S) > 0.001)
    q = prepare_known_latents(None, torch.zeros(3, 8 * S, 8 * S, 3, dtype=torch.uint8), px, 3, mask_erode=0)
    assert torch.equal(q["mask"].view(1, 4, S, S), latent_mask(px, 0)[:, None].expand(-1, 4, -1, -1)) and torch.equal(q["mask_px"], px)
    assert prepare_known_latents(None, None, None, 3) is None
    rows = torch.arange(12).view(6, 2)
    assert torch.equal(gather_rows(rows, [4, 1]), rows[[4, 1]]) and torch.equal(gather_rows(rows[:1], [4, 1]), rows[:1])


# ------------------------------------------------------------------------------ the levels
def test_known_schedule_on_the_dit_node_table(repo_root):
    import inspect
    from naturaldiffusion_amd.sampler import known_schedule, KNOWN_COLUMN0, ValidateNI
    # the levels ValidateNI.first_input (level 0) and ValidateNI.step(known=, mask=) (level k + 1) blend at
    assert {"known", "mask", "known_final"} <= set(inspect.signature(ValidateNI.step).parameters)
    assert {"known", "mask", "index", "known_final"} <= set(inspect.signature(ValidateNI.first_input).parameters)
    node = load_coeff_npz(repo_root / "results/ddpm/ddpm_024.npz")[2]
    N = node.shape[0] - 1
    assert N == 24 and np.allclose(node[:, 1] ** 2 + node[:, 2] ** 2, 1.0, atol=1e-12)   # the marginal (alpha, sigma) of every level
    assert tuple(node[0]) == (999.0, 0.0, 1.0) and tuple(node[N]) == (-1.0, 1.0, 0.0)
    lv = known_schedule(node, "mean")
    assert len(lv) == N + 1 and lv[0] == (0.0, 1.0, 2 ** 31) and KNOWN_COLUMN0 == 2 ** 31
    assert lv[N][1] == 0.0 and lv[N] == (1.0, 0.0, 2 ** 31 + N) and known_schedule(node, "data")[N] == lv[N]
    assert [c for _, _, c in lv] == [2 ** 31 + j for j in range(N + 1)]
    assert all(0.0 < s < 1.0 and 0.0 < a < 1.0 for a, s, _ in lv[1:N])
