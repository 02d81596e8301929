"""What the three generation jobs (CIFAR10, DiT, SD3) share on the host: per-image CFG scales and the guidance plan of a batch, the front end of the
inpainting arguments (the either/or refusals, the row-count rule, the reduction of a mask to one byte per latent element) and ``KnownRows``, the tables
of known data a job keeps on the host and hands to each batch.  Host code only: importing it needs no GPU and does not load the library."""
from __future__ import annotations

import numpy as np
import torch


def is_scalar_scale(cfg_scale) -> bool:
    """whether a CFG argument is one number (every image's scale) rather than a sequence with one entry per image"""
    return isinstance(cfg_scale, (int, float, np.floating, np.integer))


def job_scales(cfg_scale, sample_count):
    """The CFG scale of every image of a job, by GLOBAL index: a number is every image's scale, a sequence must have exactly
    ``sample_count`` entries (image i carries ``cfg_scale[i]`` whatever the rank, world or batch split, like its label).  Each
    is rounded to fp32, the value the step kernel multiplies by.  Pure host code."""
    sample_count = int(sample_count)
    if is_scalar_scale(cfg_scale):
        return [float(np.float32(cfg_scale))] * sample_count
    table = [float(np.float32(v)) for v in cfg_scale]
    if len(table) != sample_count:
        raise ValueError(f"{len(table)} CFG scales for {sample_count} images: a scale sequence has one entry per image of the job")
    return table


def check_interval(interval, number=float, lo: str = "s_lo", hi: str = "s_hi") -> None:
    """a guidance interval is None or a pair with lo <= hi, compared as ``number`` (int timesteps, float sigmas); ``lo`` / ``hi`` word the refusal"""
    if interval is not None and (len(interval) != 2 or number(interval[0]) > number(interval[1])):
        raise ValueError(f"guidance_interval must be ({lo}, {hi}) with {lo} <= {hi}, got {interval!r}")


def guidance_plan(levels, n_step, scales, interval=None):
    """The guidance of one batch -> (guided, slots, scales).  ``scales``: the batch's per-image CFG scales (``job_scales`` taken at the batch's
    global indices); ``levels[kk]``: the number step kk is placed by (the DiT job's timestep, the SD3 job's sigma); ``interval`` None or
    ``(lo, hi)`` on that scale, both ends inclusive.

    ``slots[i]``: the row of image i among the batch's unconditional samples, or -1 for an image whose scale is exactly 1.0 (unguided, no
    unconditional sample); the images that are guided take rows 0, 1, ... in batch order.  ``guided[kk]``: whether step kk runs the
    unconditional samples at all -- its level lies in the interval and at least one image has a slot.  A step that is not guided is unguided
    for every image.  ``scales`` comes back as the fp32 values.  At most two forward shapes per batch: n + max(slots) + 1 samples and n."""
    scales = [float(np.float32(v)) for v in scales]
    slots, g = [], 0
    for v in scales:
        slots.append(-1 if v == 1.0 else g)
        g += v != 1.0
    if interval is None:
        inside = [True] * int(n_step)
    else:
        lo, hi = interval
        inside = [lo <= levels[kk] <= hi for kk in range(int(n_step))]
    return [bool(g) and ok for ok in inside], slots, scales


def gather_rows(rows: torch.Tensor, batch) -> torch.Tensor:
    """The rows of a per-image table a batch takes, by global index, or the one shared row (the leading dimension kept)."""
    return rows[:1] if rows.shape[0] == 1 else rows[torch.as_tensor(list(batch), dtype=torch.int64)]


def gather_known(rows: torch.Tensor, batch) -> torch.Tensor:
    """``gather_rows``, flat: the form a step takes."""
    return gather_rows(rows, batch).reshape(-1)


def check_row_count(name: str, t, sample_count: int) -> None:
    """a per-image table holds one row per image of the job (row i belongs to global image index i) or one row shared by every image"""
    if t.shape[0] not in (1, int(sample_count)):
        raise ValueError(f"{name} must hold 1 row (shared) or sample_count ({int(sample_count)}) rows, not {t.shape[0]}")


def inpainting_on(known_latents, known_images, mask) -> bool:
    """The either/or rule of the latent-space inpainting arguments: none of the three -> False (inpainting off), exactly one of
    ``known_latents`` / ``known_images`` together with ``mask`` -> True, anything else is refused."""
    if known_latents is None and known_images is None and mask is None:
        return False
    if known_latents is not None and known_images is not None:
        raise ValueError("inpainting takes known_latents= or known_images=, not both")
    if mask is None:
        raise ValueError("inpainting needs mask= beside known_latents= / known_images=")
    if known_latents is None and known_images is None:
        raise ValueError("mask= needs known_latents= or known_images=")
    return True


def host_mask(mask) -> torch.Tensor:
    """a caller's mask as a CPU tensor: bool or uint8, non-zero = known"""
    mask = torch.as_tensor(mask).cpu()
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError("mask must be bool or uint8")
    return mask


def latent_mask(mask_px, erode: int = 1) -> torch.Tensor:
    """A pixel mask [K, 8S, 8S] (bool / uint8, non-zero = known) reduced to latent cells -> uint8 [K, S, S] on the CPU.  A cell is known iff
    every pixel of the (8 + 16*erode)-pixel square centred on it that lies inside the image is known: its own 8 x 8 pixels and ``erode`` rings
    of neighbouring cells (``max_pool2d`` of the UNKNOWN pixels over 8, then over 2*erode + 1 cells; the pooling pads with -inf, so what lies
    outside the image never makes a cell unknown).  Pure host code."""
    m = torch.as_tensor(mask_px).cpu()
    erode = int(erode)
    if m.dtype not in (torch.bool, torch.uint8) or m.dim() != 3 or m.shape[1] % 8 or m.shape[2] % 8 or not m.shape[1] or not m.shape[2]:
        raise ValueError("a pixel mask must be bool or uint8 [K, H, W] with H and W positive multiples of 8")
    if erode < 0:
        raise ValueError("mask_erode must be >= 0")
    u = torch.nn.functional.max_pool2d(1.0 - (m != 0).to(torch.float32)[:, None], 8)
    if erode:
        u = torch.nn.functional.max_pool2d(u, 2 * erode + 1, 1, erode)
    return (1.0 - u)[:, 0].to(torch.uint8)


def mask_table(mask: torch.Tensor, ch: int, S: int, sample_count: int, mask_erode: int = 1, forms=("element", "cell", "pixel")):
    """A ``host_mask`` for latents [ch, S, S] -> uint8 [K', ch*S*S], one byte per latent ELEMENT (the form the steps take), K' 1 or
    ``sample_count``; None when the mask has none of the accepted ``forms`` (the caller words that refusal).  ``"element"``: [K', ch, S, S] as it
    is; ``"cell"``: [K', S, S], every channel; ``"pixel"``: [K', 8S, 8S], reduced to cells by ``latent_mask(mask, mask_erode)``, every channel."""
    shape = tuple(mask.shape[1:])
    form = ("element" if mask.dim() == 4 and shape == (ch, S, S) else "cell" if mask.dim() == 3 and shape == (S, S) else
            "pixel" if mask.dim() == 3 and shape == (8 * S, 8 * S) else None)
    if form not in forms:
        return None
    check_row_count("mask", mask, sample_count)
    cells = latent_mask(mask, mask_erode) if form == "pixel" else (mask != 0).to(torch.uint8)
    if form != "element":
        cells = cells[:, None].expand(-1, ch, -1, -1)
    return cells.reshape(cells.shape[0], ch * S * S).contiguous()


class KnownRows:
    """The known data of a job on the host, named tables ``[K, ...]`` with K 1 (one row shared by every image) or one row per image, and each batch's
    flat device tensors.  A table given here is indexed by GLOBAL image index; one filled by ``encode`` holds this rank's rows only, in its order."""

    def __init__(self, device, **tables):
        self.device = device
        self.tables = dict(tables)
        self.row_of = {}                  # table name -> {global image index: row}, for the tables that hold this rank's rows only
        self._shared = {}                 # table name -> the one-row table on the device, uploaded once per job

    def encode(self, name: str, source: torch.Tensor, batches, encode_chunk, max_batch: int = 1) -> None:
        """Fill table ``name`` from ``source`` ``[K, ...]``: ``encode_chunk(rows of source, their row numbers) -> [len, E]`` on the host is asked for the
        one shared row, or for every global index in ``batches`` (this rank's index lists) once, in that order, in chunks of at most ``max_batch``."""
        shared = source.shape[0] == 1
        rows = [0] if shared else [i for b in batches for i in b]
        mb = max(1, int(max_batch))
        parts = [encode_chunk(source[torch.as_tensor(rows[s0:s0 + mb], dtype=torch.int64)], rows[s0:s0 + mb]) for s0 in range(0, len(rows), mb)]
        if parts:                         # (a rank without batches asks for nothing)
            self.tables[name] = torch.cat(parts)
            if not shared:
                self.row_of[name] = {i: r for r, i in enumerate(rows)}

    def batch(self, indices) -> dict:
        """table name -> the batch's rows, flat on the device: the rows at the batch's global indices, or the one shared row."""
        out = {}
        for name, t in self.tables.items():
            if t.shape[0] == 1:
                if name not in self._shared:
                    self._shared[name] = t.reshape(-1).to(self.device)
                out[name] = self._shared[name]
            else:
                rows = [self.row_of[name][i] for i in indices] if name in self.row_of else indices
                out[name] = gather_known(t, rows).to(self.device)
        return out
