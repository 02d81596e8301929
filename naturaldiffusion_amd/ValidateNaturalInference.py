"""Drop-in for ``src/ValidateNaturalInference.py``: original DDPM / DDIM skip samplers vs their
Natural Inference (coefficient-matrix) form, DiT-XL/2 + CFG 4.0, 24 steps, seed 0.

Same public names as the reference (``space_timesteps``, ``create_ddpm_coeff``, ``skip_ddpm_coeff``,
``create_ddim_coeff``, ``skip_ddim_coeff``, ``calc_x0_mean_z``, ``forward_cfg``, ``weighted_sum``,
``ddpm_skip_sample``, ``ddim_skip_sample``, ``natural_inference``, ``compare_output_tx``; globals
``vae_path``, ``model_path``).  ``natural_inference`` -- the path being accelerated -- runs one fused
``natinf_step_f32prod`` launch per step.  The two *original* samplers are the baselines it is compared
with and stay host-sequenced tensor algebra.  The DiT-XL/2 denoiser is the gfx950 engine of
``include/natinf_dit.h`` loaded from ``model_path`` (or whatever ``denoiser_factory`` returns); the VAE decoder is
the engine of ``include/natinf_vae.h`` loaded from ``vae_path`` (or ``decoder_factory``), images written with PIL.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Callable, List, Optional

import numpy as np
import torch

from . import _lib, jobs
from ._lib import lib, check, ptr, stream_ptr
from .coeff import load_coeff_npz, SparseRows
from .jobs import (KnownRows, check_interval, check_row_count, gather_rows, host_mask, inpainting_on, is_scalar_scale, job_scales,  # noqa: F401
                   latent_mask, mask_table)                # (job_scales, latent_mask and gather_rows: importable from here as before)
from .sampler import ValidateNI

root_path = Path(__file__).resolve().parent.parent
vae_path = None
model_path = None
device = "cuda:0"

# hooks: () -> object with .forward(z, t, y) returning [B, 8, H, W]; () -> callable(latents) -> images
denoiser_factory: Optional[Callable] = None
decoder_factory: Optional[Callable] = None
last_latents: Optional[torch.Tensor] = None      # final latents of the most recent sampler call


def make_path(path):
    path = os.path.abspath(path)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    return path


def space_timesteps(num_timesteps, section_counts):
    """Timesteps kept when striding a ``num_timesteps`` process (reference :28-79; improved-DDPM recipe)."""
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            want = int(section_counts[4:])
            for stride in range(1, num_timesteps):
                if len(range(0, num_timesteps, stride)) == want:
                    return set(range(0, num_timesteps, stride))
            raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")
        section_counts = [int(v) for v in section_counts.split(",")]
    base, extra = divmod(num_timesteps, len(section_counts))
    start, steps = 0, []
    for i, count in enumerate(section_counts):
        size = base + (1 if i < extra else 0)
        if size < count:
            raise ValueError(f"cannot divide section of {size} steps into {count}")
        stride = 1 if count <= 1 else (size - 1) / (count - 1)
        pos = 0.0
        for _ in range(count):
            steps.append(start + round(pos))
            pos += stride
        start += size
    return set(steps)


def _abar():
    betas = np.linspace(0.0001, 0.02, 1000, dtype=np.float64)
    alphas = 1 - betas
    return betas, alphas, np.cumprod(alphas)


def create_ddpm_coeff():
    """[alphas, alphas_bar, log_var, coeff_xt2x0, coeff_eps2x0, coeff_xt, coeff_x0] (reference :82-99)."""
    betas, alphas, abar = _abar()
    prev = np.append(1.0, abar[:-1])
    var = betas * (1.0 - prev) / (1.0 - abar)
    return [alphas, abar, np.log(np.append(1E-5, var[1:])), np.sqrt(1.0 / abar), np.sqrt(1.0 / abar - 1),
            np.sqrt(alphas) * (1 - prev) / (1 - abar), np.sqrt(prev) * betas / (1 - abar)]


def _skip(abar, num_step):
    idx = sorted(space_timesteps(1000, str(num_step)))
    sab = abar[idx]
    sa = np.zeros_like(sab)
    sa[0] = sab[0]
    sa[1:] = sab[1:] / sab[:-1]
    return idx, sa, sab, np.append(1.0, sab[:-1])


def skip_ddpm_coeff(coeff_all, num_step=50):
    """Re-derive the DDPM tables on the strided schedule (reference :102-133)."""
    idx, sa, sab, prev = _skip(coeff_all[1], num_step)
    sb = 1 - sa
    var = sb * (1.0 - prev) / (1.0 - sab)
    out = [sa, sab, np.log(np.append(1E-5, var[1:])), np.sqrt(1.0 / sab), np.sqrt(1.0 / sab - 1),
           np.sqrt(sa) * (1 - prev) / (1 - sab), np.sqrt(prev) * sb / (1 - sab)]
    return out, idx


def create_ddim_coeff():
    """(alphas, alphas_bar, coeff_xt2x0, coeff_eps2x0, coeff_xt, coeff_x0) (reference :136-151)."""
    _, alphas, abar = _abar()
    prev = np.append(1.0, abar[:-1])
    rect = np.sqrt((1 - prev) / (1 - abar))
    return alphas, abar, np.sqrt(1.0 / abar), np.sqrt(1.0 / abar - 1), rect, np.sqrt(prev) - rect * np.sqrt(abar)


def skip_ddim_coeff(coeff_all, num_step=50):
    """Reference :154-174."""
    idx, sa, sab, prev = _skip(coeff_all[1], num_step)
    rect = np.sqrt((1 - prev) / (1 - sab))
    return (sa, sab, np.sqrt(1.0 / sab), np.sqrt(1.0 / sab - 1), rect, np.sqrt(prev) - rect * np.sqrt(sab)), idx


def calc_x0_mean_z(input_z, eps, coeff, ii):
    """Reference :177-182."""
    coeff_xt2x0, coeff_eps2x0, coeff_xt, coeff_x0 = coeff
    x0 = coeff_xt2x0[ii] * input_z - coeff_eps2x0[ii] * eps
    return x0, coeff_xt[ii] * input_z + coeff_x0[ii] * x0


@torch.no_grad()
def _cond_uncond(model, zt, timesteps, classlabels, classnulls):
    """The two denoiser calls of a CFG step (reference :190-191).  A denoiser that takes 2n samples (the gfx950 DiT engine: ``max_batch``) gets them
    as ONE forward of [z; z] with [labels; nulls] -- at n = 8 a DiT-XL/2 forward is ~300 dependent launches of 10-30 us each, so two forwards
    of 8 cost almost twice one of 16; samples are independent inside the engine, so the halves are what the two calls return."""
    n = len(zt)
    if getattr(model, "max_batch", 0) >= 2 * n:
        both = model.forward(torch.cat([zt, zt]), torch.cat([timesteps, timesteps]), torch.cat([classlabels.to(classnulls.dtype), classnulls]))
        return both[:n], both[n:]
    return model.forward(zt, timesteps, classlabels), model.forward(zt, timesteps, classnulls)


@torch.no_grad()
def forward_cfg(model, zt, timesteps, classlabels, cfg_scale, cls):
    """Reference :185-195: two denoiser calls (batched into one where the denoiser allows), first 4 of 8 channels, CFG fuse."""
    classnulls = torch.tensor([cls] * len(zt), device=zt.device)
    cond, uncond = _cond_uncond(model, zt, timesteps, classlabels, classnulls)
    cond_eps, uncond_eps = cond[:, :4, :, :], uncond[:, :4, :, :]
    return cond_eps, uncond_eps, uncond_eps + cfg_scale * (cond_eps - uncond_eps)


@torch.no_grad()
def weighted_sum(weights, seq_elem):
    """Reference :198-204: fp32 products accumulated in fp64 -> fp32 (``natinf_weighted_sum_f32prod``)."""
    _lib.require_gpu()
    slab = torch.stack([s.contiguous().reshape(-1) for s in seq_elem]).to(torch.float32)
    n, E = slab.shape
    rows = SparseRows(np.asarray(weights, np.float64)[None, :n], lambda k: n, torch.float32, slab.device, dense=True, diag=False)
    out = torch.empty(E, dtype=torch.float32, device=slab.device)
    idx, val, nt = rows.ptrs(0)
    check(lib.natinf_weighted_sum_f32prod(ptr(slab), ptr(out), idx, val, nt, E, stream_ptr()), "natinf_weighted_sum_f32prod")
    return out.view(seq_elem[0].shape)


_engine_cache = {}


def load_dit_engine(path, max_batch=16, fp8=False, stream16=None):
    """Reference :150-154 (``DiT_models['DiT-XL/2'](input_size=32, num_classes=1000)`` + ``load_state_dict``) on the
    gfx950 engine: the checkpoint's tensors go straight into ``natinf_dit_load``; one engine per checkpoint path and
    input size.  The input size is the checkpoint's own (``pos_embed``): 32 for ``DiT-XL-2-256x256.pt``, 64 for
    ``DiT-XL-2-512x512.pt``.  ``fp8``: the engine's fp8 projections (include/natinf_dit.h, NATINF_DIT_FP8); the two modes
    are two engines.  ``stream16``: None = the library's default residual-stream format, True / False = IEEE half / fp32, ``"auto"`` = the
    half stream with the stream guard (``DiTEngine(..., stream16=True, guard=True)``: what ``generate_sharded(stream16="auto")`` runs first); one
    engine per mode, like ``fp8``."""
    from .dit import DiTEngine, flatten_state_dict, input_size_of, XL2
    if stream16 not in (None, True, False, "auto"):
        raise ValueError(f'stream16 must be None, True, False or "auto", got {stream16!r}')
    sd = None
    size = _engine_sizes.get(str(path))
    if size is None:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        size = _engine_sizes[str(path)] = input_size_of(sd)
    key = (str(path), max_batch, size, bool(fp8)) + (() if stream16 is None else (stream16,))
    if key not in _engine_cache:
        if sd is None:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        _engine_cache[key] = DiTEngine(flatten_state_dict(sd, XL2["depth"], XL2["hidden"], size), max_batch, device=device,
                                       input_size=size, fp8=bool(fp8), stream16=True if stream16 == "auto" else stream16, guard=stream16 == "auto", **XL2)
    return _engine_cache[key]


_engine_sizes = {}


def latent_size(model) -> int:
    """Latent side S of the denoiser in use: the engine's ``input_size``; 32 for a denoiser that declares none."""
    return int(getattr(model, "input_size", 32))


def _setup(seed):
    torch.manual_seed(seed)
    torch.set_grad_enabled(False)
    model, _ = _resolve_denoiser(None, None, 8, False, None)               # the factory's, or the engine of model_path for 2 x 8 samples
    labels = torch.tensor([207, 360, 387, 974, 88, 979, 417, 279], device=device)
    return model, labels, len(labels)


def _read_vae_weights(path):
    """state dict of an AutoencoderKL: ``path`` is the model directory (``diffusion_pytorch_model.safetensors`` / ``.bin``) or a weights file"""
    p = Path(path)
    if p.is_dir():
        cand = [p / "diffusion_pytorch_model.safetensors", p / "diffusion_pytorch_model.bin"]
        p = next((c for c in cand if c.exists()), cand[0])
    if p.suffix == ".safetensors":
        from safetensors.torch import load_file
        return load_file(str(p))
    return torch.load(p, map_location="cpu", weights_only=True)


def load_vae_decoder(path, max_batch=8, latent_res=32):
    """Reference :212-214 (``AutoencoderKL.from_pretrained(vae_path)``) on the gfx950 decoder engine (include/natinf_vae.h):
    ``path`` is the model directory (``diffusion_pytorch_model.safetensors`` / ``.bin``) or a weights file; one engine
    per latent resolution (32: 256x256 images, 64: 512x512)."""
    from .vae import VAEDecoder, flatten_state_dict
    key = ("vae", str(path), max_batch, latent_res)
    if key not in _engine_cache:
        _engine_cache[key] = VAEDecoder(flatten_state_dict(_read_vae_weights(path), 4, prefix="decoder."), max_batch, latent_ch=4, latent_res=latent_res, device=device)
    return _engine_cache[key]


def load_vae_encoder(path, max_batch=16, latent_res=32):
    """The other half of the same AutoencoderKL weights file on the gfx950 encoder engine (``vae.encode`` of
    src/AnalyzeWeightedSumDegradation.py:56): ``path`` as for ``load_vae_decoder``; one engine per latent resolution
    (32: 256x256 images, 64: 512x512)."""
    from .vae import VAEEncoder, flatten_encoder_state_dict
    key = ("vae_enc", str(path), max_batch, latent_res)
    if key not in _engine_cache:
        _engine_cache[key] = VAEEncoder(flatten_encoder_state_dict(_read_vae_weights(path), 4, prefix="encoder."), max_batch, latent_ch=4, latent_res=latent_res, device=device)
    return _engine_cache[key]


_png_pool = None


def write_png_rgb(arr: np.ndarray, path, level: int = 1, threads: int = 8) -> None:
    """An 8-bit RGB PNG of ``arr`` [H, W, 3] uint8, deflated in ``threads`` row bands at once.  The file is what any PNG reader decodes to the same pixels: filter
    type 0 on every row, ONE zlib stream assembled from independently compressed bands (each band a raw deflate stream closed by a byte-aligned sync flush, the
    last one finished; the zlib header and the Adler-32 of the whole filtered image around them -- the way pigz builds a stream).  Why: the 2066 x 260 row of eight
    256 x 256 images is 1.6 MB of poorly compressible pixels, and PIL's single-threaded encoder took 51-62 ms for it on the GPU box's host -- a quarter of a 24-step
    Validate run of 8 images on the DiT engine, all of it behind the last kernel.  ``zlib.compress`` releases the GIL, so the bands really run side by side."""
    import struct
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    a = np.ascontiguousarray(arr, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("write_png_rgb expects [H, W, 3] uint8")
    h, w = int(a.shape[0]), int(a.shape[1])
    raw = np.zeros((h, 1 + 3 * w), np.uint8)                          # filter byte 0 (None) in front of every row
    raw[:, 1:] = a.reshape(h, 3 * w)
    nb = max(1, min(int(threads), h // 16 if h >= 16 else 1))
    cuts = [h * i // nb for i in range(nb + 1)]
    bands = [raw[cuts[i]:cuts[i + 1]].tobytes() for i in range(nb)]

    def deflate(i):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)                # raw deflate
        return c.compress(bands[i]) + c.flush(zlib.Z_FINISH if i == nb - 1 else zlib.Z_SYNC_FLUSH)
    if nb > 1:
        global _png_pool
        if _png_pool is None:                                         # (kept: starting eight threads costs as much as they save on one image row)
            _png_pool = ThreadPoolExecutor(max(8, nb), thread_name_prefix="natinf-png")
        parts = list(_png_pool.map(deflate, range(nb)))
    else:
        parts = [deflate(0)]
    adler = 1
    for b in bands:
        adler = zlib.adler32(b, adler)
    idat = b"\x78\x01" + b"".join(parts) + struct.pack(">I", adler & 0xffffffff)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(str(path), "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", idat) + chunk(b"IEND", b""))


def save_image_grid(images: torch.Tensor, path, nrow: int = 8) -> None:
    """``torchvision.utils.save_image(samples, path, nrow=8, normalize=True, value_range=(-1, 1))`` (reference :236; the 8
    validation images come out as one row of 8) without
    torchvision: clamp to [-1, 1], map to [0, 255], tile with 2-pixel padding -- the same pixels -- and write the PNG with ``write_png_rgb`` (lossless, like
    torchvision's PIL writer; deflated at level 1 in parallel row bands instead of level 6 on one thread: 51-62 -> a few ms on the GPU box's host)."""
    # the pixel arithmetic where the tensor lives (on the device for the engines' output: 1.5 MB of uint8 cross to the host instead of 6 MB of fp32, and no
    # OpenMP team of the host's torch spins up behind the last kernel -- under a container's CPU quota that team, not the work, was what stalled a run); the same
    # fp32 operations in the same order as save_image's normalize + make_grid + mul(255).add_(0.5).clamp_(0, 255).to(uint8); pad pixels are 0
    x = images.detach().float()
    u8 = ((((x.clamp(-1, 1) + 1) * 0.5) * 255 + 0.5).clamp(0, 255)).to(torch.uint8).cpu().numpy()
    n, c, h, w = u8.shape
    ncol = min(nrow, n); nr = (n + ncol - 1) // ncol
    arr = np.zeros((nr * (h + 2) + 2, ncol * (w + 2) + 2, 3), np.uint8)
    for i in range(n):
        r0, c0 = (i // ncol) * (h + 2) + 2, (i % ncol) * (w + 2) + 2
        arr[r0:r0 + h, c0:c0 + w, :] = np.transpose(u8[i], (1, 2, 0)) if c == 3 else np.repeat(np.transpose(u8[i], (1, 2, 0)), 3, axis=2)
    write_png_rgb(arr, path, threads=4)


def _finish(input_z, name):
    global last_latents
    last_latents = input_z
    S = input_z.shape[-1]
    if S != 32:                                              # (256x256 keeps the reference's names; other sizes must not overwrite them)
        name = name[:-4] + "__%dx%d.png" % (8 * S, 8 * S)
    if decoder_factory is not None:
        decoder_factory()(input_z / 0.18215, make_path(root_path / ("results/validation/" + name)))
    elif vae_path is not None:                               # reference :231-236: decode the latents, write the 1x8 image row
        images = load_vae_decoder(vae_path, latent_res=S)(input_z / 0.18215)
        save_image_grid(images, make_path(root_path / ("results/validation/" + name)))
    return input_z


def _original(num_step, stochastic, seed=0):
    model, labels, n = _setup(seed)
    tables, skip_idxs = (skip_ddpm_coeff(create_ddpm_coeff(), num_step) if stochastic
                         else skip_ddim_coeff(create_ddim_coeff(), num_step))
    tb = [torch.from_numpy(e).to(device=device, dtype=torch.float32) for e in tables]
    log_var = tb[2] if stochastic else None
    coeff = tuple(tb[3:7]) if stochastic else tuple(tb[2:6])
    S = latent_size(model)
    input_z = torch.randn(n, 4, S, S, device=device)
    for ii in list(range(0, num_step))[::-1]:
        timesteps = torch.ones(n, dtype=torch.int32, device=device) * skip_idxs[ii]
        _, _, fuse_eps = forward_cfg(model, input_z, timesteps, labels, 4.0, 1000)
        _, mean_z = calc_x0_mean_z(input_z, fuse_eps, coeff, ii)
        if stochastic:
            noise = torch.randn_like(input_z, dtype=torch.float32, device=device)
            input_z = mean_z + torch.exp(0.5 * log_var[ii]) * noise
        else:
            input_z = mean_z
    return input_z


def ddpm_skip_sample(num_step=24):
    """Reference :207-256 (the classical ancestral sampler NI is compared with)."""
    return _finish(_original(num_step, True), "ddpm_%03d__seed_%d__original.png" % (num_step, 0))


@torch.no_grad()
def ddim_skip_sample(num_step=24):
    """Reference :259-308."""
    return _finish(_original(num_step, False), "ddim_%03d__seed_%d__original.png" % (num_step, 0))


def natural_inference(alg_name="ddpm", num_step=24):
    """Reference :311-372 on the fused kernel: per step two denoiser calls, one fresh ``randn_like`` written
    straight into the noise-history slab, one ``natinf_step_f32prod`` launch."""
    model, labels, n = _setup(0)
    weight_path = root_path / ("results/%s/%s_%03d.npz" % (alg_name.replace("_sympy", ""), alg_name, num_step))
    C, B, node = load_coeff_npz(weight_path)
    num_step = B.shape[0]
    tables, _ = skip_ddim_coeff(create_ddim_coeff(), num_step)
    c1 = np.asarray(tables[2])[::-1]
    c2 = np.asarray(tables[3])[::-1]
    S = latent_size(model)
    E = n * 4 * S * S
    ni = ValidateNI(C, B, node, c1.astype(np.float32), c2.astype(np.float32), E, device=device)
    noise = torch.randn(n, 4, S, S, device=device)
    ni.hist_eps[0].copy_(noise.reshape(-1))
    input_z = noise.clone()
    classnulls = torch.full((n,), 1000, dtype=labels.dtype, device=device)             # (reference :352 builds it per step from a host list: a blocking copy each time)
    for kk in range(num_step):
        timesteps = torch.full((n,), int(node[kk, 0]), dtype=torch.int32, device=device)
        cond, uncond = _cond_uncond(model, input_z, timesteps, labels, classnulls)      # [n, 8, S, S] each; first 4 channels used
        ni.hist_eps[kk + 1].copy_(torch.randn_like(input_z, dtype=torch.float32, device=device).reshape(-1))
        per, stride = 4 * S * S, cond.shape[1] * S * S
        z = ni.step(kk, input_z.reshape(-1), cond.contiguous(), uncond.contiguous(), 4.0, per, stride)
        input_z = z.view(n, 4, S, S)
    weight_name = os.path.basename(weight_path)[:-4]
    return _finish(input_z.clone(), "%s__seed_%d__natural.png" % (weight_name, 0))


DEMO_LABELS = (207, 360, 387, 974, 88, 979, 417, 279)     # reference :156: the eight ImageNet classes of the demo row


def job_batches(sample_count, batch_size, rank=0, world=1, labels=None):
    """The batches rank ``rank`` of ``world`` generates: a list of (global image indices, class labels).  Indices are sharded
    like the other two paths (``shard.rank_batches``: rank r owns r, r+world, ...; only a rank's last batch is ragged).  The
    label of an image is a function of its GLOBAL index alone, so it is the same image under any split: ``labels`` None
    cycles the reference's eight demo labels (indices 0-7 are the demo row), a sequence of ``sample_count`` entries is taken
    per index, a shorter one is cycled.  1000 is the null class of the unconditional half, so a label outside 0..999 is an
    error.  Pure host code."""
    from .shard import rank_batches
    sample_count, batch_size = int(sample_count), int(batch_size)
    if sample_count < 0 or batch_size <= 0:
        raise ValueError("sample_count must be >= 0 and batch_size positive")
    table = [int(v) for v in (DEMO_LABELS if labels is None else labels)]
    if not table:
        raise ValueError("labels must not be empty")
    if len(table) > sample_count and labels is not None:
        raise ValueError(f"{len(table)} labels for {sample_count} images")
    bad = [v for v in table if not 0 <= v <= 999]
    if bad:
        raise ValueError(f"class labels must be in 0..999 (1000 is the null class of the unconditional half), got {bad[0]}")
    return [(idx, [table[i % len(table)] for i in idx]) for idx in rank_batches(sample_count, batch_size, rank, world)]


def guidance_plan(node, n_step, scales, interval=None):
    """The guidance of one batch -> (guided, slots, scales): ``jobs.guidance_plan``, which describes the three, on the timestep scale.  ``interval``
    None or ``(t_lo, t_hi)``, integers on the scale of the timestep the job feeds the denoiser at step kk, ``int(node[kk, 0])``, both ends
    inclusive; an unguided image (scale exactly 1.0, slot -1) is eps = cond, with no unconditional sample.  Pure host code."""
    return jobs.guidance_plan([int(node[kk, 0]) for kk in range(int(n_step))], n_step, scales, None if interval is None else tuple(int(v) for v in interval))


def to_pixels_u8(images: torch.Tensor) -> torch.Tensor:
    """[n, 3, H, W] decoder output -> [n, H, W, 3] uint8 where the tensor lives: ``save_image_grid``'s pixel expression."""
    x = images.detach().float()
    return ((((x.clamp(-1, 1) + 1) * 0.5) * 255 + 0.5).clamp(0, 255)).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def prepare_known_latents(known_latents, known_images, mask, sample_count: int, known_final: str = "mean", mask_erode: int = 1):
    """The inpainting arguments of ``generate_sharded``, checked and brought to one form -> None (inpainting off) or a dict: ``S`` (the latent
    side they imply), ``mask`` (uint8 [K', 4*S*S] per latent ELEMENT, the form the step takes), and either ``latents`` (fp32 [K, 4*S*S]) or
    ``images`` (the caller's uint8 [K, 8S, 8S, 3] / fp32 [K, 3, 8S, 8S], still to be encoded) with ``mask_px`` (bool [K', 8S, 8S]); K and K' each
    ``sample_count`` (row i belongs to global image index i) or 1 (shared by every image).  Pure host code: every refusal comes before any GPU
    call."""
    if not inpainting_on(known_latents, known_images, mask):
        return None
    if known_final not in ("mean", "data"):
        raise ValueError('known_final must be "mean" or "data"')
    sample_count = int(sample_count)
    mask = host_mask(mask)
    if known_latents is not None:
        kl = torch.as_tensor(known_latents).cpu()
        if kl.dtype != torch.float32 or kl.dim() != 4 or kl.shape[1] != 4 or kl.shape[2] != kl.shape[3] or kl.shape[2] % 2 or not kl.shape[2]:
            raise ValueError("known_latents must be fp32 [K, 4, S, S] in the denoiser's scale")
        S = int(kl.shape[2])
        check_row_count("known_latents", kl, sample_count)
        table = mask_table(mask, 4, S, sample_count, forms=("element", "cell"))
        if table is None:
            raise ValueError(f"with known_latents the mask must be [K', {S}, {S}] (a latent cell: every channel) or [K', 4, {S}, {S}]")
        return dict(S=S, latents=kl.reshape(kl.shape[0], -1).contiguous(), mask=table)
    ki = torch.as_tensor(known_images).cpu()
    if not (ki.dim() == 4 and ((ki.dtype == torch.uint8 and ki.shape[3] == 3 and ki.shape[1] == ki.shape[2]) or
                               (ki.dtype == torch.float32 and ki.shape[1] == 3 and ki.shape[2] == ki.shape[3]))):
        raise ValueError("known_images must be uint8 [K, 8S, 8S, 3] or fp32 [K, 3, 8S, 8S] in [-1, 1]")
    R = int(ki.shape[2])                                              # the side, in either form
    if not R or R % 16:
        raise ValueError("known_images must be 8S pixels on a side, S even")
    check_row_count("known_images", ki, sample_count)
    table = mask_table(mask, 4, R // 8, sample_count, mask_erode, forms=("pixel",))
    if table is None:
        raise ValueError(f"with known_images the mask must be a pixel mask [K', {R}, {R}]")
    return dict(S=R // 8, images=ki, mask_px=mask != 0, mask=table)


def _resolve_denoiser(model, fallback, batch_size, fp8, stream16):
    """the denoiser of a job or a sampler and, for ``stream16="auto"``, the callable that builds its fp32-stream twin -> (model, fallback)"""
    auto = stream16 == "auto"
    if auto and fallback is None and model_path is not None and model is None and denoiser_factory is None:
        fallback = lambda: load_dit_engine(model_path, max_batch=2 * batch_size, fp8=fp8, stream16=False)
    if model is None:
        if denoiser_factory is not None:
            model = denoiser_factory()
        elif model_path is not None:
            model = load_dit_engine(model_path, max_batch=2 * batch_size, fp8=fp8, stream16=stream16)
        else:
            raise RuntimeError("set ValidateNaturalInference.model_path (a DiT-XL/2 state dict, reference :152-154) or "
                               "ValidateNaturalInference.denoiser_factory (generate_sharded also takes model=); see INTEGRATION.md")
    if fp8 and not getattr(model, "fp8", False):
        raise ValueError("fp8=True, but the denoiser given is not an fp8 engine (DiTEngine(..., fp8=True))")
    if auto and not (getattr(model, "guard", False) and hasattr(model, "stream_status")):
        raise ValueError('stream16="auto" needs a guarded denoiser (DiTEngine(..., guard=True)): an unguarded one cannot say that it overflowed')
    if auto and fallback is None:
        raise ValueError('stream16="auto" with a denoiser of the caller\'s needs fallback=: a callable that returns the fp32-stream denoiser')
    return model, fallback


def _resolve_decoder(decoder, decode, decode_batch, S):
    """the decoder of a job: the one given, else ``decoder_factory()``, else the VAE engine of ``vae_path``; None with none of them or ``decode=False``"""
    if decode and decoder is None and decoder_factory is not None:
        return decoder_factory()
    if decode and decoder is None and vae_path is not None:
        return load_vae_decoder(vae_path, max_batch=int(decode_batch), latent_res=S)
    return decoder if decode else None


def _known_rows(inpaint, batches, encoder, S) -> KnownRows:
    """``prepare_known_latents``' tables as ``KnownRows``; ``known_images`` are encoded here, to the posterior mean in the denoiser's scale"""
    if inpaint["S"] != S:
        raise ValueError(f"the known data is for latents of side {inpaint['S']}, the denoiser's are {S}")
    if "latents" in inpaint:
        return KnownRows(device, known=inpaint["latents"], mask=inpaint["mask"])
    from .AnalyzeWeightedSumDegradation import preprocess
    if encoder is None:
        if vae_path is None:
            raise RuntimeError("known_images= needs encoder= or ValidateNaturalInference.vae_path (load_vae_encoder)")
        encoder = load_vae_encoder(vae_path, latent_res=S)

    def encode_chunk(chunk, rows):
        x = (preprocess(chunk) if chunk.dtype == torch.uint8 else chunk).to(device)
        return encoder.encode(x, sample=False, scale=0.18215, index=rows).reshape(len(chunk), -1).cpu()
    known = KnownRows(device, mask=inpaint["mask"])
    known.encode("known", inpaint["images"], [idx for idx, _ in batches], encode_chunk, getattr(encoder, "max_batch", 1))
    return known


def _first_z(ni, noise, index, blend):
    """the first model input of a trajectory: the noise, or (inpainting) the noise with the known latents at level 0; ``noise`` stays eps_0"""
    return ni.first_input(noise.reshape(-1), index=index, **blend).view(noise.shape) if blend else noise


def _trajectory(denoiser, ni, noise, index, steps_t, classlabels, classnulls, cfg_scale, blend):
    """one batch in the default form: [z; z] forwards and the launch-wide step; ``blend``: the batch's known= / mask= / known_final= ({}: none)"""
    shape, S = noise.shape, noise.shape[-1]
    per = 4 * S * S
    input_z, flat_noise = _first_z(ni, noise, index, blend), noise.reshape(-1)
    for kk in range(len(steps_t)):
        cond, uncond = _cond_uncond(denoiser, input_z, steps_t[kk], classlabels, classnulls)   # [n, 8, S, S] each; first 4 channels used
        z = ni.step(kk, input_z.reshape(-1), cond.contiguous(), uncond.contiguous(), cfg_scale, per, cond.shape[1] * S * S,
                    noise=flat_noise, index=index, **blend)
        input_z = z.view(shape)
    return input_z.clone()


def _batch_plan(node, n_step, scales, interval, classlabels, classnulls):
    """the ``guidance_plan`` of a batch with its device tensors, built once per batch (the rerun of a clamped batch uses the same plan)"""
    dev = classlabels.device
    guided, slots, scales = guidance_plan(node, n_step, scales, interval)
    pick = [i for i, s in enumerate(slots) if s >= 0]
    n, g = len(slots), len(pick)
    return (guided, torch.tensor(pick, dtype=torch.int64, device=dev), torch.cat([classlabels, classnulls[:g]]),
            [torch.full((n + g,), int(node[kk, 0]), dtype=torch.int32, device=dev) for kk in range(n_step)],
            torch.tensor(slots, dtype=torch.int32, device=dev), torch.tensor(scales, dtype=torch.float32, device=dev))


def _planned_trajectory(denoiser, ni, noise, index, steps_t, classlabels, plan, blend):
    """``_trajectory`` under a ``_batch_plan``: a guided step forwards [z; z[G]] (one call when the denoiser takes n + |G| samples) and makes the
    per-image step, every other step forwards the n conditional samples alone"""
    guided, pick, labels_g, steps_g, slots_t, scales_t = plan
    shape, n, g, S = noise.shape, noise.shape[0], len(pick), noise.shape[-1]
    per = 4 * S * S
    joint = getattr(denoiser, "max_batch", 0) >= n + g
    nulls = labels_g[n:]
    input_z, flat_noise = _first_z(ni, noise, index, blend), noise.reshape(-1)
    for kk in range(len(steps_t)):
        if not guided[kk]:
            cond = denoiser.forward(input_z, steps_t[kk], classlabels).contiguous()
            z = ni.step(kk, input_z.reshape(-1), cond, None, 1.0, per, cond.shape[1] * S * S, noise=flat_noise, index=index, **blend)
        else:
            zg = input_z if g == n else input_z[pick]
            if joint:
                both = denoiser.forward(torch.cat([input_z, zg]), steps_g[kk], labels_g).contiguous()
                cond, uncond = both[:n], both[n:]
            else:
                cond = denoiser.forward(input_z, steps_t[kk], classlabels).contiguous()
                uncond = denoiser.forward(zg, steps_g[kk][n:], nulls).contiguous()
            z = ni.step(kk, input_z.reshape(-1), cond, uncond, scales_t, per, cond.shape[1] * S * S, noise=flat_noise, index=index,
                        uncond_slot=slots_t, n_uncond=g, **blend)
        input_z = z.view(shape)
    return input_z.clone()


def _guarded_batch(trajectory, model, wide, fallback, args, report, bi):
    """One batch of a ``stream16="auto"`` job -> (latents, the fp32-stream denoiser once built): the status is reset in front of the batch and read
    once behind it (the job's one wait per batch); a batch that clamped runs again, with the same arguments, on ``wide``."""
    model.reset_stream_status()
    latents = trajectory(model, *args)
    st = model.stream_status()
    hit = np.flatnonzero(np.asarray(st["clamped"]))
    if len(hit):
        if report["first_clamp"] is None:
            k = int(hit[0])
            report["first_clamp"] = dict(batch=bi, site=k, site_name=model.site_names[k], max_abs=float(st["max_abs"][k]), clamped=int(st["clamped"][k]))
        report["rerun_batches"].append(bi)
        if wide is None:
            wide = fallback()
        latents = trajectory(wide, *args)                                 # same noise, same labels, same indices: the fp32-stream job's batch
    return latents, wide


def _decode_images(decoder, latents, indices, labels, decode_batch, image_sink, pasted):
    """decode in chunks of ``decode_batch`` -> uint8 images on the CPU, or None when ``image_sink`` takes each chunk; ``pasted``: None, or the
    caller's (pixel mask, uint8 images) by global index, whose known pixels go back into the decoded images first"""
    db, out = max(1, int(decode_batch)), []
    for s0 in range(0, len(indices), db):
        u8 = to_pixels_u8(decoder(latents[s0:s0 + db] / 0.18215))
        if pasted is not None:
            u8 = torch.where(gather_rows(pasted[0], indices[s0:s0 + db]).to(device)[..., None], gather_rows(pasted[1], indices[s0:s0 + db]).to(device), u8)
        if image_sink is not None:
            image_sink(u8, indices[s0:s0 + db], labels[s0:s0 + db])
        else:
            out.append(u8.cpu())
    if image_sink is not None:
        return None
    return torch.cat(out) if out else torch.empty((0, 8 * latents.shape[-1], 8 * latents.shape[-1], 3), dtype=torch.uint8)


@torch.no_grad()
def generate_sharded(sample_count, labels=None, alg_name="ddpm", num_step=24, batch_size=32, rank=0, world=1, seed=0,
                     cfg_scale=4.0, decode=True, decode_batch=8, model=None, decoder=None, image_sink=None, fp8=False, stream16=None,
                     fallback=None, report=None, guidance_interval=None, known_latents=None, known_images=None, mask=None,
                     known_final="mean", mask_erode=1, paste=True, encoder=None):
    """A class-conditional generation job on the loop of ``natural_inference`` (reference :311-372): ``sample_count`` images,
    image i of class ``job_batches``' label of i, sharded by global index over ``world`` ranks with no collective on the data
    path.  The noise is counter-based: z_0 = eps_0 = ``philox_noise(indices, column=0)`` and the noise a stochastic matrix
    injects after step j-1 is drawn inside the fused step from Philox(seed, global index, column j)
    (natinf_step_f32prod_noise), so image i is the same trajectory for any batch size or GPU count wherever the denoiser
    itself is batch-independent.  Per step: ONE denoiser forward of [z; z] with [labels; 1000...] and one step launch;
    nothing in the loop waits for the GPU.

    ``model`` None: ``denoiser_factory()`` or the engine of ``model_path`` built for ``2*batch_size`` samples -- with
    ``fp8`` its fp8-projection form (``load_dit_engine(..., fp8=True)``; a ``model`` or factory given carries its own mode).  ``decoder``
    None: ``decoder_factory()`` or the VAE engine of ``vae_path`` (here a callable latents/0.18215 -> images in [-1, 1]); with
    neither, or ``decode=False``, no image is made.  Decoding runs in chunks of ``decode_batch``; ``image_sink(images uint8
    [n, 8S, 8S, 3] on the device, indices, labels)``, when given, gets each chunk instead of the images being collected.

    ``stream16`` None / True / False: the residual-stream format of the engine built from ``model_path`` (``load_dit_engine``; a ``model`` or factory given
    carries its own).  ``"auto"``: every batch runs on a GUARDED half-stream engine (``model`` given: it must be one, ``DiTEngine(..., guard=True)``) whose status is
    reset in front of the batch and read once behind its last step; a batch in which any update left the half range (a ``clamped`` counter is not zero) is run again
    on the fp32-stream engine -- ``fallback()``, or ``load_dit_engine(model_path, ..., stream16=False)``, built at the first such batch -- and, the noise being a
    function of (seed, global index, column), the rerun IS the fp32-stream job's batch.  ``report`` (a dict, filled): ``batches``, ``rerun_batches`` (positions in
    this rank's batch list), ``first_clamp`` ({batch, site, site_name, max_abs, clamped} or None).  A ``report`` given is filled in every mode; without ``"auto"`` nothing is monitored, so it
    says ``rerun_batches == []`` and ``first_clamp is None`` whatever the stream did.

    Guidance.  ``cfg_scale`` a float and ``guidance_interval`` None (the defaults' form) is the reference's one hard-wired form and makes exactly the calls
    it always made: every step a forward of [z; z] and natinf_step_f32prod_noise with the one scale -- byte-identical latents.  Two arguments go beyond it
    (``guidance_plan``, natinf_step_f32prod_noise_guided):

    * ``cfg_scale`` a sequence of ``sample_count`` floats, by GLOBAL image index: image i carries its own scale whatever the rank, world or batch split.  A scale
      exactly 1.0 means unguided: no unconditional sample for that image at any step, eps = cond.
    * ``guidance_interval=(t_lo, t_hi)``: guide only at the steps whose timestep ``int(node[kk, 0])`` (what the denoiser is fed) lies in t_lo..t_hi, both ends
      inclusive; every other step is unguided for every image (Kynkaanniemi et al., 2024).  With it a scalar ``cfg_scale == 1.0`` means unguided as well.

    With G the guided images of a batch at a step: G empty -> ONE forward of the n conditional samples and the step with ``uncond=None``; otherwise one forward
    of [z; z[G]] with [labels; 1000 x |G|] and the guided step, slots 0..|G|-1 at the positions in G and -1 elsewhere.  Slot and scale tensors are built once
    per batch; nothing in the loop waits for the GPU beyond the slot read-back the C entry makes.  Contract: with either new argument image i is still a
    function of (seed, global index, its label, its scale, the interval) up to the denoiser's own batch dependence -- the same function, not the same bytes as
    the default form: the engine picks GEMM tile variants by row count, so a forward of n + |G| rows and one of 2n may differ by bf16 rounding flips (DESIGN.md 4d
    records the same caveat for the VAE).  ``stream16="auto"``, ``fp8``, ``image_sink``, ``report`` and ``fallback`` compose unchanged; the rerun of a clamped
    batch uses the same plan.

    Inpainting in latent space.  Exactly one of ``known_latents`` / ``known_images``, together with ``mask``, switches it on; without
    them the job makes exactly the calls described above.  The first model input is the noise with the known latents diffused to level 0
    (``ValidateNI.first_input``), and every step overwrites the known latent elements, inside its one launch (natinf_step_f32prod_inpaint), with the known
    latents diffused to the level of its output: ``known_schedule`` of the node table, the draws keyed by (seed, global index, column 2^31 + level).
    ``known_final``: ``"mean"`` leaves alpha_N * known behind the last step (alpha_N is 1 in the DiT tables), ``"data"`` the known latents as given.

    * ``known_latents``: fp32 ``[K, 4, S, S]`` in the denoiser's scale (already x 0.18215), K 1 (shared) or ``sample_count`` (row i belongs to global index
      i).  ``mask``: bool / uint8 ``[K', S, S]`` (a cell: all four channels) or ``[K', 4, S, S]``, K' 1 or ``sample_count``; non-zero = known.  No encoder.
    * ``known_images``: uint8 ``[K, 8S, 8S, 3]`` (the job's own output format) or fp32 ``[K, 3, 8S, 8S]`` in [-1, 1], encoded once per job (the rows this
      rank generates, in chunks of the encoder's ``max_batch``) by ``encoder``, else ``load_vae_encoder(vae_path, latent_res=S)``, to the posterior MEAN x
      0.18215.  ``mask`` is then a pixel mask ``[K', 8S, 8S]``, reduced to cells by ``latent_mask(mask, mask_erode)``: a cell is known iff every pixel of the
      (8 + 16*mask_erode)-pixel square around it is.  The encoder's receptive field is wider than a cell, so the known cells next to the hole still carry
      some of whatever the caller left IN the hole; ``mask_erode`` trades known area for less of that.  It is a knob, not a guarantee.
    * ``paste`` (uint8 ``known_images`` only; ignored with ``known_latents`` or fp32 images): the decoded uint8 images get the caller's known pixels back,
      ``where(mask, known, decoded)`` on the caller's PIXEL mask, before ``image_sink`` / collection.

    Contract: image i is a function of (seed, global index, label, scale, its known row and mask row) up to the denoiser's own batch dependence.  Both the
    default and the planned (guidance) form take it, the ``stream16="auto"`` rerun uses the same known rows, and ``fp8``, ``image_sink``, ``report`` and
    ``guidance_interval`` compose unchanged.

    -> (latents [n_local, 4, S, S] fp32 on the device, labels [n_local] int64 CPU, global indices [n_local] int64 CPU,
        images [n_local, 8S, 8S, 3] uint8 CPU or None)"""
    from .CIFAR10NaturalInference import philox_noise
    torch.set_grad_enabled(False)
    batch_size = int(batch_size)
    batches = job_batches(sample_count, batch_size, rank, world, labels)
    inpaint = prepare_known_latents(known_latents, known_images, mask, sample_count, known_final, mask_erode)   # refusals before any GPU call
    planned = guidance_interval is not None or not is_scalar_scale(cfg_scale)   # False: the reference's form, today's calls
    scale_of = job_scales(cfg_scale, sample_count) if planned else None
    check_interval(guidance_interval, int, "t_lo", "t_hi")
    if stream16 not in (None, True, False, "auto"):
        raise ValueError(f'stream16 must be None, True, False or "auto", got {stream16!r}')
    auto = stream16 == "auto"
    model, fallback = _resolve_denoiser(model, fallback, batch_size, fp8, stream16)
    if report is None:
        report = {}
    report.update(batches=len(batches), rerun_batches=[], first_clamp=None)
    S = latent_size(model)
    decoder = _resolve_decoder(decoder, decode, decode_batch, S)
    weight_path = root_path / ("results/%s/%s_%03d.npz" % (alg_name.replace("_sympy", ""), alg_name, num_step))
    C, B, node = load_coeff_npz(weight_path)
    n_step = B.shape[0]
    tables, _ = skip_ddim_coeff(create_ddim_coeff(), n_step)
    c1 = np.asarray(tables[2])[::-1].astype(np.float32)
    c2 = np.asarray(tables[3])[::-1].astype(np.float32)
    per = 4 * S * S
    known = None if inpaint is None else _known_rows(inpaint, batches, encoder, S)
    trajectory = _planned_trajectory if planned else _trajectory
    samplers, out_z = {}, []                                          # batch size -> ValidateNI (the ragged last batch gets its own)
    wide = None                                                       # the fp32-stream denoiser: built at the first batch that needs it
    for bi, (indices, labs) in enumerate(batches):
        n = len(indices)
        if n not in samplers:
            samplers[n] = ValidateNI(C, B, node, c1, c2, n * per, device=device, seed=seed, elems_per_image=per)
        index = torch.tensor(indices, dtype=torch.int64, device=device)
        classlabels = torch.tensor(labs, dtype=torch.int64, device=device)
        classnulls = torch.full((n,), 1000, dtype=torch.int64, device=device)
        steps_t = [torch.full((n,), int(node[kk, 0]), dtype=torch.int32, device=device) for kk in range(n_step)]
        noise = philox_noise(indices, (4, S, S), seed, device, column=0)
        # the batch's known rows by global index, gathered on the host, uploaded on the caller's stream ({}: no inpainting, today's calls)
        blend = {} if known is None else dict(known.batch(indices), known_final=known_final)
        guidance = (_batch_plan(node, n_step, [scale_of[i] for i in indices], guidance_interval, classlabels, classnulls),) if planned else (classnulls, float(cfg_scale))
        args = (samplers[n], noise, index, steps_t, classlabels) + guidance + (blend,)
        if auto:
            latents_b, wide = _guarded_batch(trajectory, model, wide, fallback, args, report, bi)
        else:
            latents_b = trajectory(model, *args)
        out_z.append(latents_b)
    latents = torch.cat(out_z) if out_z else torch.empty((0, 4, S, S), dtype=torch.float32, device=device)
    all_idx = [i for idx, _ in batches for i in idx]
    all_lab = [l for _, lb in batches for l in lb]
    images = None
    if decoder is not None:
        pasted = paste and inpaint is not None and "images" in inpaint and inpaint["images"].dtype == torch.uint8   # the caller's known pixels back
        images = _decode_images(decoder, latents, all_idx, all_lab, decode_batch, image_sink, (inpaint["mask_px"], inpaint["images"]) if pasted else None)
    return latents, torch.tensor(all_lab, dtype=torch.int64), torch.tensor(all_idx, dtype=torch.int64), images


def compare_output_tx():
    ddpm_skip_sample(24)
    ddim_skip_sample(24)
    natural_inference("ddpm_sympy", 24)
    natural_inference("ddim_sympy", 24)


if __name__ == "__main__":
    vae_path = "./sd-vae-ft-ema"
    model_path = "./DiT-XL-2-256x256.pt"
    compare_output_tx()
