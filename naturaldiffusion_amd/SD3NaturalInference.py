"""Drop-in for ``src/SD3NaturalInference.py``: SD3-medium, 28 steps, CFG 7, fp16, seed 10, n = 4.

Public names as in the reference: ``weighted_sum(seq_xstarts, weights=None)``, ``euler_weighted_sum``,
``sd_natural_inference_tx()``, ``sd_euler_natural_inference_tx()``.  Per step the two MMDiT calls are
followed by ONE fused launch (``natinf_step_f16chain``: x0 from velocity, CFG fuse, append, row-normalised
fp16 weighted mean, next model input).  The text encoders / scheduler / VAE are third-party (``diffusers``,
un-vendored and unpinned in the reference); a ``pipe`` object with the same attributes can be passed in.  The
denoiser ``pipe.transformer`` is replaced by the gfx950 MMDiT engine (``use_native_transformer``; on by default when
the pipe is loaded here): text and null prompts then go through ONE batched forward per step.
The reference's 28x5x4 intermediate VAE decodes (:223-236, visualisation only) are off by default.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ptr, stream_ptr
from .coeff import load_sd3_csv, SparseRows
from .jobs import KnownRows, check_interval, check_row_count, guidance_plan, host_mask, inpainting_on, is_scalar_scale, job_scales, mask_table
from .sampler import SD3NI

root_path = Path(__file__).resolve().parent.parent
results_path = root_path            # where results/sd3/*.png go (the reference writes below its own root, :241)
PROMPT = "A cat holding a sign that says hello world"


def weighted_sum(seq_xstarts: Sequence[torch.Tensor], weights=None) -> torch.Tensor:
    """Reference :157-168: fp16 chain, row ``len(seq)-1`` of ``weights`` (uniform mean if None)."""
    _lib.require_gpu()
    n = len(seq_xstarts)
    slab = torch.stack([s.contiguous().reshape(-1) for s in seq_xstarts]).to(torch.float16)
    E = slab.shape[1]
    row = np.ones((1, n)) if weights is None else np.asarray(weights, np.float64)[n - 1:n, :n]
    rows = SparseRows(row, lambda k: n, torch.float32, slab.device, dense=True, diag=False)
    out = torch.empty(E, dtype=torch.float16, device=slab.device)
    idx, val, nt = rows.ptrs(0)
    check(lib.natinf_weighted_mean_f16(ptr(slab), ptr(out), idx, val, nt, rows.rows[0].total, E, stream_ptr()),
          "natinf_weighted_mean_f16")
    return out.view(seq_xstarts[0].shape)


def euler_weighted_sum(seq_xstarts, cliplen=0):
    """Reference :61-69: ``seq_xstarts`` = [(weight 0-d tensor, x0)], returns (acc, acc/sum_w) in fp16 ops."""
    _lib.require_gpu()
    seq = seq_xstarts[-cliplen:]
    n = len(seq)
    slab = torch.stack([x.contiguous().reshape(-1) for _, x in seq]).to(torch.float16)
    E = slab.shape[1]
    h = lambda t: float(torch.as_tensor(t, dtype=torch.float32).to(torch.float16))
    tot = 0
    for w, _ in seq:
        tot = tot + torch.as_tensor(w, dtype=torch.float32).cpu()
    row = np.array([[h(torch.as_tensor(w).cpu()) for w, _ in seq]])
    rows = SparseRows(row, lambda k: n, torch.float32, slab.device, dense=True, diag=False)
    idx, val, nt = rows.ptrs(0)
    acc = torch.empty(E, dtype=torch.float16, device=slab.device)
    mean = torch.empty(E, dtype=torch.float16, device=slab.device)
    check(lib.natinf_weighted_mean_f16(ptr(slab), ptr(acc), idx, val, nt, 1.0, E, stream_ptr()), "natinf_weighted_mean_f16")
    # `acc / acc_weight`: a 0-d fp32 divisor keeps its fp32 value (it is only cast to fp16 as a FIRST operand)
    check(lib.natinf_weighted_mean_f16(ptr(slab), ptr(mean), idx, val, nt, float(tot), E, stream_ptr()), "natinf_weighted_mean_f16")
    shape = seq[0][1].shape
    return acc.view(shape), mean.view(shape)


def use_native_transformer(pipe, n: int, latent_side: int = 128, ctx_tokens: Optional[int] = None, device="cuda:0"):
    """Swap ``pipe.transformer`` (diffusers ``SD3Transformer2DModel``) for the HIP engine built from its own weights
    (include/natinf_mmdit.h).  ``n`` = images per batch; the engine is sized for the 2n sequences of a CFG step."""
    from .mmdit import MMDiTEngine, flatten_state_dict
    tr = pipe.transformer
    if isinstance(tr, MMDiTEngine):
        return pipe
    cfg = tr.config
    kw = dict(layers=cfg.num_layers, heads=cfg.num_attention_heads, joint_dim=cfg.joint_attention_dim,
              pooled_dim=cfg.pooled_projection_dim, in_ch=cfg.in_channels)
    if cfg.attention_head_dim != 64 or cfg.patch_size != 2:
        raise ValueError("the engine supports head_dim 64 / patch 2 (SD3-medium)")
    grid = latent_side // 2
    if ctx_tokens is None:
        ctx_tokens = 77 + 256                               # CLIP (77) + T5 (max_sequence_length 256): encode_prompt's default
    flat = flatten_state_dict(tr.state_dict(), grid, **kw)
    pipe.transformer = MMDiTEngine(flat, max_batch=2 * n, grid=grid, ctx_tokens=ctx_tokens, device=device, **kw)
    return pipe


def use_native_vae(pipe, n: int, latent_side: int = 128, device="cuda:0"):
    """Decode with the HIP AutoencoderKL decoder engine (include/natinf_vae.h) built from ``pipe.vae``'s own weights instead of
    ``pipe.vae.decode`` (reference :238-240); ``pipe.vae`` stays in place for its config (scaling / shift factors)."""
    from .vae import VAEDecoder, flatten_state_dict
    if getattr(pipe, "natinf_vae", None) is None:
        lc = int(pipe.vae.config.latent_channels)
        pipe.natinf_vae = VAEDecoder(flatten_state_dict(pipe.vae.state_dict(), lc, prefix="decoder."), max_batch=n,
                                     latent_ch=lc, latent_res=latent_side, device=device)
    return pipe


def use_native_vae_encoder(pipe, n: int, latent_side: int = 64, device="cuda:0"):
    """Encode with the HIP AutoencoderKL encoder engine (include/natinf_vae.h) built from ``pipe.vae``'s own weights; ``pipe.vae`` stays in place for
    its config.  ``pipe.natinf_vae_encoder`` is the engine, for ``n`` images of ``8 * latent_side`` pixels a side; the engine's own size limit
    (``latent_side`` <= 64) holds."""
    from .vae import VAEEncoder, flatten_encoder_state_dict
    enc = getattr(pipe, "natinf_vae_encoder", None)
    if enc is None or enc.latent_res != int(latent_side) or enc.max_batch < int(n):
        lc = int(pipe.vae.config.latent_channels)
        pipe.natinf_vae_encoder = VAEEncoder(flatten_encoder_state_dict(pipe.vae.state_dict(), lc, prefix="encoder."), max_batch=int(n),
                                             latent_ch=lc, latent_res=int(latent_side), device=device)
    return pipe


def sd_prepare_known(known_latents, known_images, mask, sample_count, latent_shape, renoise: str = "fresh", mask_erode: int = 1):
    """The inpainting arguments of ``sd_generate_sharded``, checked and brought to one form -> None (inpainting off) or a dict: ``mask`` (uint8
    [K', C*H*W], one byte per latent ELEMENT, the form the step takes) and either ``latents`` (fp16 [K, C*H*W]) or ``images`` (the caller's uint8
    [K, 8H, 8W, 3] / fp32 [K, 3, 8H, 8W], still to be encoded); K and K' each ``sample_count`` (row i belongs to global image index i) or 1 (shared
    by every image).  Pure host code: every refusal comes before any GPU call."""
    given = known_latents is not None or known_images is not None or mask is not None
    if given and sample_count is None:
        raise ValueError("known_latents / known_images / mask need sample_count (the reference's job generates from noise alone)")
    inpainting_on(known_latents, known_images, mask)
    if renoise not in ("fresh", "same"):
        raise ValueError('renoise must be "fresh" or "same"')
    if not given:
        return None
    sample_count = int(sample_count)
    shape = tuple(int(v) for v in latent_shape)
    if len(shape) != 3 or shape[1] != shape[2]:
        raise ValueError(f"inpainting needs a square latent_shape (C, S, S), not {shape}")
    ch, S, _ = shape
    out = dict(mask=mask_table(host_mask(mask), ch, S, sample_count, mask_erode))
    if out["mask"] is None:
        raise ValueError(f"mask must be a latent-element mask [K', {ch}, {S}, {S}], a cell mask [K', {S}, {S}] or a pixel mask [K', {8 * S}, {8 * S}]")
    if known_latents is not None:
        kl = torch.as_tensor(known_latents).cpu()
        if not kl.is_floating_point() or kl.dim() != 4 or tuple(kl.shape[1:]) != shape:
            raise ValueError(f"known_latents must be floating point [K, {ch}, {S}, {S}] in the model's space, (z - shift) * scale")
        check_row_count("known_latents", kl, sample_count)
        out["latents"] = kl.to(torch.float16).reshape(kl.shape[0], ch * S * S).contiguous()
        return out
    ki = torch.as_tensor(known_images).cpu()
    R = 8 * S
    if S > 64:
        raise ValueError(f"known_images of {R} pixels a side: the encoder engine stops at 512 (latent side 64); pass known_latents= instead")
    if not ((ki.dtype == torch.uint8 and ki.dim() == 4 and tuple(ki.shape[1:]) == (R, R, 3)) or
            (ki.dtype == torch.float32 and ki.dim() == 4 and tuple(ki.shape[1:]) == (3, R, R))):
        raise ValueError(f"known_images must be uint8 [K, {R}, {R}, 3] or fp32 [K, 3, {R}, {R}] in [-1, 1]")
    check_row_count("known_images", ki, sample_count)
    out["images"] = ki
    return out


def _known_rows(pipe, inpaint, batches, n, S, device) -> KnownRows:
    """``sd_prepare_known``'s tables as ``KnownRows``; ``known_images`` are encoded here through the encoder engine built from ``pipe.vae``
    (``use_native_vae_encoder``) to fp16 on the host: the posterior MEAN in the model's space, (z - shift) * scale."""
    if "latents" in inpaint:
        return KnownRows(device, known=inpaint["latents"], mask=inpaint["mask"])
    from .AnalyzeWeightedSumDegradation import preprocess
    enc = use_native_vae_encoder(pipe, n, S, device).natinf_vae_encoder
    scale, shift = float(pipe.vae.config.scaling_factor), float(getattr(pipe.vae.config, "shift_factor", 0.0) or 0.0)

    def encode_chunk(chunk, rows):
        x = (preprocess(chunk) if chunk.dtype == torch.uint8 else chunk).to(device)
        return enc.encode(x, sample=False, scale=scale, shift=shift).reshape(len(chunk), -1).to(torch.float16).cpu()
    known = KnownRows(device, mask=inpaint["mask"])
    known.encode("known", inpaint["images"], batches, encode_chunk, enc.max_batch)
    return known


def _load_pipe(pipe, device, dtype, n=4):
    if pipe is not None:
        return pipe
    try:
        from diffusers import StableDiffusion3Pipeline
    except ImportError as e:
        raise ImportError("SD3 needs the `diffusers` package and the stabilityai/stable-diffusion-3-medium-diffusers "
                          "weights (un-vendored in the reference); pass pipe=... to use another denoiser") from e
    pipe = StableDiffusion3Pipeline.from_pretrained("stabilityai/stable-diffusion-3-medium-diffusers",
                                                    torch_dtype=dtype, local_files_only=True).to(device)
    return use_native_vae(use_native_transformer(pipe, n, device=device), n, device=device)


def philox_noise_f16(indices, shape_per_image=(16, 128, 128), seed: int = 10, device="cuda:0") -> torch.Tensor:
    """fp16 N(0,1) latents, image i keyed by its GLOBAL index (include/natinf.h natinf_randn_philox_f32, rounded to fp16 once): the
    same image for any GPU count / batch split -- the sharded counterpart of the reference's one ``torch.randn(n, 16, 128, 128)`` (:184-186),
    as ``CIFAR10NaturalInference.philox_noise`` is for config 3."""
    from .CIFAR10NaturalInference import philox_noise
    return philox_noise(indices, shape_per_image, seed, device).to(torch.float16)


def _prepare(pipe, device, dtype, n, seed, num_step, noises):
    prompts = [PROMPT] * n
    if noises is None:
        generator = torch.Generator(device)
        generator.manual_seed(seed)
        noises = torch.randn(n, 16, 128, 128, device=device, dtype=dtype, generator=generator)
    emb = pipe.encode_prompt(prompt=prompts, prompt_2=None, prompt_3=None, negative_prompt="")
    pipe.scheduler.set_timesteps(num_step, device=device)
    return noises, emb, pipe.scheduler.timesteps.to(device), pipe.scheduler.sigmas.to(device)


def _decode(pipe, latents):
    """Reference :238-240 -> list of uint8 HWC RGB arrays (the pixels ``image_processor.postprocess(output_type="pil")`` holds:
    ``(x / 2 + 0.5).clamp(0, 1) * 255`` rounded)."""
    z = (latents / pipe.vae.config.scaling_factor) + pipe.vae.config.shift_factor
    dec = getattr(pipe, "natinf_vae", None)
    if dec is not None:
        images = dec(z.float())
        return list(((images * 0.5 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy())
    images = pipe.vae.decode(z, return_dict=False)[0]
    return [np.array(im) for im in pipe.image_processor.postprocess(images, output_type="pil")]


def _write_row(path, images):
    """Reference :241-243 (``cv2.imwrite`` of the BGR-flipped row of images) without cv2: the same RGB file through PIL."""
    from PIL import Image
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    Image.fromarray(np.hstack(images)).save(str(path))


def _velocity(pipe, x, ts, text, pooled, joint):
    """one denoiser call on the sequences given: the engine's own ``forward`` when it holds them (``joint``), the reference's call shape otherwise"""
    if joint:
        return pipe.transformer.forward(x, ts, text, pooled)
    return pipe.transformer(hidden_states=x, timestep=ts, encoder_hidden_states=text, pooled_projections=pooled, return_dict=False)[0]


def _velocities(pipe, x, ts, emb):
    """the text and null velocities of a step: ONE forward when the transformer is the engine and holds 2n sequences, the reference's two calls otherwise"""
    pe, ne, ppe, npe = emb
    from .mmdit import MMDiTEngine
    n = x.shape[0]
    if isinstance(pipe.transformer, MMDiTEngine) and pipe.transformer.max_batch >= 2 * n:
        v = _velocity(pipe, torch.cat([x, x]), torch.cat([ts, ts]), torch.cat([pe, ne]), torch.cat([ppe, npe]), True)
        return v[:n].contiguous(), v[n:].contiguous()
    return _velocity(pipe, x, ts, pe, ppe, False).contiguous(), _velocity(pipe, x, ts, ne, npe, False).contiguous()


def _default_trajectory(pipe, ni, noises, timesteps, num_step, emb):
    """The reference's loop (:198-223) for one batch in the default form -> the mean behind the last step, ``noises``' shape, the sampler's own
    buffer: the flow input, then per step the two velocities of [x; x] and one natinf_step_f16chain launch with the sampler's one scale."""
    shape = noises.shape
    flat_noise = noises.contiguous().reshape(-1)
    x = ni.first_input(flat_noise)
    for kk in range(num_step):
        vt, vn = _velocities(pipe, x.view(shape), timesteps[kk].expand(shape[0]), emb)
        mean, x = ni.step(kk, x, vt.reshape(-1), vn.reshape(-1), flat_noise, want_next=kk + 1 < num_step)
    return mean.view(shape)


def job_prompts(prompts, sample_count):
    """The prompt of every image of a job, by GLOBAL index: None is ``PROMPT`` for every image, a string is every image's prompt, a
    sequence must hold exactly ``sample_count`` strings (image i carries ``prompts[i]`` whatever the rank, world or batch split).
    Pure host code."""
    sample_count = int(sample_count)
    if prompts is None or isinstance(prompts, str):
        return [PROMPT if prompts is None else prompts] * sample_count
    table = list(prompts)
    if len(table) != sample_count or not all(isinstance(p, str) for p in table):
        raise ValueError(f"{len(table)} prompts for {sample_count} images: a prompt sequence has one string per image of the job")
    return table


def sd_guidance_plan(sigmas, n_step, scales, interval=None):
    """The guidance of one batch -> (guided, slots, scales): ``jobs.guidance_plan``, which describes the three, on the sigma scale.  ``interval`` None
    or ``(s_lo, s_hi)``: step kk is inside when ``s_lo <= float(sigmas[kk]) <= s_hi``, the fp32 value of the schedule the step multiplies by, both
    ends inclusive; an unguided image (scale exactly 1.0, slot -1) is f = x - sig*v_text, with no null-prompt sequence.  Pure host code."""
    check_interval(interval)
    n_step = int(n_step)
    if len(sigmas) < n_step:
        raise ValueError(f"{len(sigmas)} sigmas for {n_step} steps")
    return guidance_plan([float(sigmas[kk]) for kk in range(n_step)], n_step, scales, None if interval is None else tuple(float(v) for v in interval))


def _planned_trajectory(pipe, ni, noises, timesteps, num_step, emb, plan, blend=None):
    """The loop of ``sd_generate_sharded`` under an ``sd_guidance_plan``: a guided step forwards [x; x[G]] with [pe; ne[G]] and [ppe; npe[G]] (one call
    when the transformer is the engine and takes n + |G| sequences, two otherwise) and makes the per-image step; every other step forwards the n text
    sequences alone and makes the per-image step with every slot -1.  ``blend`` (inpainting: ``known``, ``mask``, ``seed``, ``index``, ``renoise`` of
    ``SD3NI.step``) goes to the first input and to every step; the last step, whose mean is the result, blends the mean."""
    from .mmdit import MMDiTEngine
    blend = blend or {}
    guided, pick, slots_t, none_t, scales_t = plan
    pe, ne, ppe, npe = emb
    nb, g, per = noises.shape[0], pick.numel(), noises[0].numel()
    engine = isinstance(pipe.transformer, MMDiTEngine)
    joint = engine and pipe.transformer.max_batch >= nb + g
    alone = engine and pipe.transformer.max_batch >= nb
    if g:
        ne_g, npe_g = (ne, npe) if g == nb else (ne[pick], npe[pick])
        text_g, pooled_g = torch.cat([pe, ne_g]), torch.cat([ppe, npe_g])
    flat_noise = noises.reshape(-1)
    x = ni.first_input(flat_noise, sample_elems=per, **blend) if blend else ni.first_input(flat_noise)
    for kk in range(num_step):
        xs, want = x.view(noises.shape), kk + 1 < num_step
        step_kw = dict(blend, blend_mean=not want) if blend else {}
        if not guided[kk]:
            vt = _velocity(pipe, xs, timesteps[kk].expand(nb), pe, ppe, alone).contiguous()
            mean, x = ni.step(kk, x, vt.reshape(-1), None, flat_noise, want_next=want, cfg=scales_t, uncond_slot=none_t, n_uncond=0, sample_elems=per, **step_kw)
            continue
        xg = xs if g == nb else xs[pick]
        if joint:
            v = pipe.transformer.forward(torch.cat([xs, xg]), timesteps[kk].expand(nb + g), text_g, pooled_g)
            vt, vn = v[:nb].contiguous(), v[nb:].contiguous()
        else:
            vt = _velocity(pipe, xs, timesteps[kk].expand(nb), pe, ppe, alone).contiguous()
            vn = _velocity(pipe, xg, timesteps[kk].expand(g), ne_g, npe_g, engine and pipe.transformer.max_batch >= g).contiguous()
        mean, x = ni.step(kk, x, vt.reshape(-1), vn.reshape(-1), flat_noise, want_next=want, cfg=scales_t, uncond_slot=slots_t, n_uncond=g, sample_elems=per, **step_kw)
    return mean


@torch.no_grad()
def sd_generate_sharded(pipe, sample_count: int, n: int = 4, rank: int = 0, world: int = 1, seed: int = 10, num_step: int = 28,
                        weight_name: str = "sd3_step_28_weight.csv", device="cuda:0", latent_shape=(16, 128, 128), *,
                        prompts=None, negative_prompt: str = "", cfg_scale=7.0, guidance_interval=None,
                        known_latents=None, known_images=None, mask=None, renoise: str = "fresh", mask_erode: int = 1):
    """Batch-sharded SD3 generation (BASELINE configs 4 / 5): this rank runs the reference's loop (:198-223) for the images
    whose GLOBAL index is rank, rank + world, ... in batches of ``n`` -- no collective on the data path, Philox noise keyed by the global index
    (``philox_noise_f16``), so image i is the same bytes whatever the GPU count or batch split.  ``pipe`` as in ``sd_natural_inference_tx``
    (``encode_prompt`` is asked for ``n`` prompts once; a ragged last batch uses the first rows).

    Prompts.  ``prompts`` None (the default) is the reference's one ``PROMPT`` for every image, encoded once as above.  A string gives every image that
    prompt; a sequence must hold exactly ``sample_count`` strings, by GLOBAL image index (``job_prompts``).  With either, ``encode_prompt`` is called once
    per batch with that batch's prompts.  ``negative_prompt`` is what ``encode_prompt`` is given for the null side (one string for the job).

    Guidance.  ``cfg_scale`` a number and ``guidance_interval`` None (the defaults' form) is the reference's one hard-wired form and makes exactly the calls
    it always made: every step a forward of [x; x] and natinf_step_f16chain with the one scale -- byte-identical latents.  Two arguments go beyond it
    (``sd_guidance_plan``, natinf_step_f16chain_guided):

    * ``cfg_scale`` a sequence of ``sample_count`` numbers, by GLOBAL image index (``jobs.job_scales``): image i carries its own scale
      whatever the rank, world or batch split.  A scale exactly 1.0 means unguided: no null-prompt sequence for that image at any step, f = x - sig*v_text.
    * ``guidance_interval=(s_lo, s_hi)`` on the sigma scale: guide only at the steps kk with ``s_lo <= float(sigmas[kk]) <= s_hi`` (the fp32 value of the
      schedule), both ends inclusive; every other step is unguided for every image (Kynkaanniemi et al., 2024).  With it a scalar ``cfg_scale == 1.0``
      means unguided as well.

    With G the guided images of a batch at a step: G empty -> ONE forward of the n text sequences and the guided step with every slot -1 (``v_null=None``,
    ``n_uncond=0``); otherwise one forward of [x; x[G]] with [pe; ne[G]] and [ppe; npe[G]] -- n + |G| <= 2n sequences, within the engine's ``max_batch`` --
    and the guided step, slots 0..|G|-1 at the positions in G and -1 elsewhere.  A transformer that is not the ``MMDiTEngine``, or one too small, gets two
    calls.  Slot and scale tensors are built once per batch; nothing in the loop waits for the GPU beyond the slot read-back the C entry makes.
    Contract: with either new argument image i is still a function of (seed, global index, its prompt, its scale, the interval) up to the engine's own
    batch dependence -- the same function, not the same bytes as the default form: the engine picks GEMM tile variants by row count, so a forward of
    n + |G| sequences and one of 2n may differ by bf16 rounding flips.  Only when n + |G| == 2n at every step (every image guided, no interval) are the
    forward shapes those of the default form, and then the kernel's identity rule makes the latents byte-identical to it.

    Inpainting in latent space.  Exactly one of ``known_latents`` / ``known_images``, together with ``mask``, switches it on; without
    them the job makes exactly the calls described above.  The first model input is the flow input with the known latents at level 0
    (``SD3NI.first_input``), and every step overwrites the known elements of its ``x_next``, inside its one launch (natinf_step_f16chain_inpaint), with
    ``sig_next*n + (1 - sig_next)*known`` in the reference's fp16 rounding order (``sd_known_schedule``).  ``renoise="fresh"`` draws n anew at every level,
    keyed by (seed, global index, column 2^31 + level); ``"same"`` uses the image's own initial noise.  The job's result is the mean, so the last step
    blends the mean: the returned latents equal ``known`` exactly at the masked elements.

    * ``known_latents``: ``[K, *latent_shape]`` in the model's space, that is already ``(z - shift) * scale``; K 1 (shared) or ``sample_count`` (row i
      belongs to global index i).  Used as fp16.
    * ``known_images``: uint8 ``[K, 8S, 8S, 3]`` or fp32 ``[K, 3, 8S, 8S]`` in [-1, 1], encoded once per job, before the loop (the rows this rank
      generates), by the encoder engine built from ``pipe.vae`` (``use_native_vae_encoder``) to the posterior MEAN, with ``scale=scaling_factor`` and
      ``shift=shift_factor``.  The encoder engine stops at latent side 64 (512 x 512 images); beyond it pass ``known_latents``.
    * ``mask`` (bool / uint8, non-zero = known; K' 1 or ``sample_count``): a latent-element mask ``[K', *latent_shape]`` as it is, a cell mask
      ``[K', S, S]`` for every channel, or a pixel mask ``[K', 8S, 8S]`` reduced by ``jobs.latent_mask(mask, mask_erode)`` and
      broadcast over the channels.

    Inpainting always runs the per-image step: a scalar ``cfg_scale`` becomes a uniform scale sequence, whose forwards are those of the default form and
    whose unknown side is, by the kernel's identity rule, the launch-wide entry's bytes.  Guidance intervals, per-image scales and prompts, fp8 engines and
    sharding compose unchanged.  Contract: image i is a function of (seed, global index, its prompt, its scale, its known row and mask row), the same
    bytes for any rank, world or batch split whenever the forward shapes agree (the caveat above).

    Returns (final latents [n_local, *latent_shape] fp16 on the device, their global indices [n_local] int64 on the CPU)."""
    from .shard import rank_batches
    inpaint = sd_prepare_known(known_latents, known_images, mask, sample_count, latent_shape, renoise, mask_erode)   # refusals before any GPU call
    planned = inpaint is not None or guidance_interval is not None or not is_scalar_scale(cfg_scale)   # False: the reference's form, today's calls
    check_interval(guidance_interval)
    if inpaint is not None and is_scalar_scale(cfg_scale):
        cfg_scale = [float(cfg_scale)] * int(sample_count)               # the uniform sequence: the default form's forwards and, on the unknown side, its bytes
    scale_of = job_scales(cfg_scale, sample_count) if planned else None
    prompt_of = None if prompts is None else job_prompts(prompts, sample_count)
    _lib.require_gpu()
    dev = torch.device(device)
    batches = list(rank_batches(sample_count, n, rank, world))
    if not batches:
        return torch.empty((0,) + tuple(latent_shape), dtype=torch.float16, device=dev), torch.empty(0, dtype=torch.int64)
    if prompt_of is None:
        emb = pipe.encode_prompt(prompt=[PROMPT] * n, prompt_2=None, prompt_3=None, negative_prompt=negative_prompt)
    pipe.scheduler.set_timesteps(num_step, device=dev)
    timesteps, sigmas = pipe.scheduler.timesteps.to(dev), pipe.scheduler.sigmas.to(dev)
    weights = load_sd3_csv(os.path.join(root_path / "weights", weight_name))
    samplers, outs = {}, []
    if planned:
        sigmas_host = sigmas.detach().to("cpu", torch.float32)
    known = None if inpaint is None else _known_rows(pipe, inpaint, batches, n, int(latent_shape[-1]), dev)   # images are encoded here, before the loop
    for batch in batches:
        nb = len(batch)
        noises = philox_noise_f16(batch, latent_shape, seed, dev)
        # inpainting: the batch's rows by global index, gathered on the host
        blend = None if known is None else dict(known.batch(batch), seed=seed, index=torch.tensor(list(batch), dtype=torch.int64, device=dev), renoise=renoise)
        if nb not in samplers:                                          # (a ragged last batch gets its own history slabs)
            samplers[nb] = SD3NI(weights, sigmas, noises.numel(), device=dev, cfg=float(cfg_scale) if not planned else 7.0,
                                 elems_per_image=noises[0].numel() if planned else None)
        if prompt_of is None:
            ni, e = samplers[nb], tuple(t[:nb] for t in emb)
        else:                                                           # this batch's prompts, by global index
            ni, e = samplers[nb], tuple(pipe.encode_prompt(prompt=[prompt_of[i] for i in batch], prompt_2=None, prompt_3=None,
                                                           negative_prompt=negative_prompt))
        if planned:                                                     # slot and scale tensors once per batch
            guided, slots, scales = sd_guidance_plan(sigmas_host, num_step, [scale_of[i] for i in batch], guidance_interval)
            plan = (guided, torch.tensor([i for i, sl in enumerate(slots) if sl >= 0], dtype=torch.int64, device=dev),
                    torch.tensor(slots, dtype=torch.int32, device=dev), torch.full((nb,), -1, dtype=torch.int32, device=dev),
                    torch.tensor(scales, dtype=torch.float32, device=dev))
            outs.append(_planned_trajectory(pipe, ni, noises, timesteps, num_step, e, plan, blend).view(noises.shape).clone())
        else:
            outs.append(_default_trajectory(pipe, ni, noises, timesteps, num_step, e).clone())
    return torch.cat(outs), torch.cat([torch.tensor(b, dtype=torch.int64) for b in batches])


@torch.no_grad()
def sd_natural_inference_tx(pipe=None, device="cuda", noises: Optional[torch.Tensor] = None, n: int = 4, seed: int = 10,
                            num_step: int = 28, weight_names=("sd3_step_28_weight.csv", "sd3_step_28_weight_sharp.csv"),
                            decode: bool = True, rank: int = 0, world: int = 1, sample_count: Optional[int] = None, latent_shape=None, *,
                            prompts=None, negative_prompt: str = "", cfg_scale=7.0, guidance_interval=None,
                            known_latents=None, known_images=None, mask=None, renoise: str = "fresh", mask_erode: int = 1):
    """Reference :172-245.  Returns the final latents per weight file (and writes ``results/sd3/sgl_*.png``
    when ``decode``).  With ``sample_count`` (not in the reference: its job is one batch of four) the job is ``sample_count`` images sharded by
    global index over ``world`` ranks (``sd_generate_sharded``): returns [(latents of this rank, global indices)] per weight file and, when
    ``decode``, writes this rank's images to ``results/sd3/sgl_<weights>_<index>.png``.  ``latent_shape`` of the sharded job: the native
    transformer's own (in_ch, 2 grid, 2 grid) when ``pipe.transformer`` is the HIP engine, the reference's (16, 128, 128) otherwise.
    ``prompts``, ``negative_prompt``, ``cfg_scale`` and ``guidance_interval`` belong to the sharded job and go to ``sd_generate_sharded`` as they are
    (per-image prompts and CFG scales by global index, a guidance interval on the sigma scale); without ``sample_count`` they are refused.  So are
    ``known_latents`` / ``known_images``, ``mask``, ``renoise`` and ``mask_erode``: latent-space inpainting, a job argument as well."""
    dtype = torch.float16
    if sample_count is None and (known_latents is not None or known_images is not None or mask is not None or renoise != "fresh" or mask_erode != 1):
        raise ValueError("known_latents / known_images / mask / renoise / mask_erode need sample_count (the reference's job generates from noise alone)")
    pipe = _load_pipe(pipe, device, dtype, n)
    if sample_count is not None:
        if latent_shape is None:
            tr = getattr(pipe, "transformer", None)
            latent_shape = (tr.in_ch, 2 * tr.grid, 2 * tr.grid) if hasattr(tr, "in_ch") and hasattr(tr, "grid") else (16, 128, 128)
        finals = []
        # an index-less "cuda" (this function's default) is THIS rank's current device -- where `_load_pipe` and the engine live after the launcher's
        # `torch.cuda.set_device(local_rank)` -- never a literal cuda:0: rank r's Philox noise and history slabs belong next to rank r's transformer
        dev_r = torch.device(device)
        if dev_r.type == "cuda" and dev_r.index is None:
            dev_r = torch.device("cuda", torch.cuda.current_device())
        for weight_name in weight_names:
            lat, idx = sd_generate_sharded(pipe, sample_count, n, rank, world, seed, num_step, weight_name, dev_r, latent_shape=tuple(latent_shape),
                                           prompts=prompts, negative_prompt=negative_prompt, cfg_scale=cfg_scale, guidance_interval=guidance_interval,
                                           known_latents=known_latents, known_images=known_images, mask=mask, renoise=renoise, mask_erode=mask_erode)
            finals.append((lat, idx))
            if decode:
                for s0 in range(0, lat.shape[0], n):
                    for im, gi in zip(_decode(pipe, lat[s0:s0 + n]), idx[s0:s0 + n].tolist()):
                        _write_row(results_path / ("results/sd3/sgl_%s_%06d.png" % (weight_name[:-4], gi)), [im])
        return finals
    if world != 1 or rank != 0:
        raise ValueError("rank / world need sample_count (the reference's job is one batch: nothing to shard)")
    if prompts is not None or negative_prompt != "" or guidance_interval is not None or not is_scalar_scale(cfg_scale) or cfg_scale != 7.0:
        raise ValueError("prompts / negative_prompt / cfg_scale / guidance_interval need sample_count (the reference's job hard-wires one prompt and cfg 7)")
    noises, emb, timesteps, sigmas = _prepare(pipe, device, dtype, n, seed, num_step, noises)
    finals = []
    for weight_name in weight_names:
        weights = load_sd3_csv(os.path.join(root_path / "weights", weight_name))
        ni = SD3NI(weights, sigmas, noises.numel(), device=noises.device, cfg=7.0)
        out = _default_trajectory(pipe, ni, noises, timesteps, num_step, emb).clone()
        finals.append(out)
        if decode:
            _write_row(results_path / ("results/sd3/sgl_%s.png" % (weight_name[:-4])), _decode(pipe, out))
    return finals


@torch.no_grad()
def sd_euler_natural_inference_tx(pipe=None, device="cuda", noises: Optional[torch.Tensor] = None, n: int = 4,
                                  seed: int = 10, num_step: int = 28, decode: bool = True) -> torch.Tensor:
    """Reference :81-154 with ``is_vanilla_update = False``: flow-Euler written as Natural Inference."""
    dtype = torch.float16
    pipe = _load_pipe(pipe, device, dtype, n)
    noises, emb, timesteps, sigmas = _prepare(pipe, device, dtype, n, seed, num_step, noises)
    ni = SD3NI(None, sigmas, noises.numel(), device=noises.device, cfg=7.0, euler=True)
    out = _default_trajectory(pipe, ni, noises, timesteps, num_step, emb).clone()
    if decode:
        _write_row(results_path / "results/sd3/euler_sgl_clip0.png", _decode(pipe, out))
    return out


if __name__ == "__main__":
    sd_natural_inference_tx()
