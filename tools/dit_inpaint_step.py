"""Time of the inpainting step of the Validate form (natinf_step_f32prod_inpaint: natinf_step_f32prod_noise_guided plus the known-latent blend in
registers) beside natinf_step_f32prod_noise_guided itself, the baseline, at E = 64 x 4096 (a job batch of 64 latents of 4 x 32 x 32) on two rows of
results/ddpm/ddpm_024.npz: row 1 (one history row and the diagonal, 3 noise terms) and row 22, the longest (22 history rows and the diagonal, 24 noise
terms of which 23 are drawn in the kernel; row 23, the last, is the diagonal and one noise term).  cond / uncond are the first 4 of 8 channels of a
[64, 8, 32, 32] tensor, every image guided (slots 0..63).  Mask fractions 0, 1/2 (the left half of every latent) and 1; at each the blend once with a
draw (std of the row's own level) and once without (std 0, what the last step of a job does).  Both entries run in one process: `windows` windows per
variant, alternating variant by variant, each a HIP-event pair around `reps` back-to-back calls after `warmup` calls; the median window is reported
with the min and max.  Both entries read their noise row and slots back before they launch, so a window holds that host work too: it is the same for
both.  The 5 B per element the blend adds (4 B known, 1 B mask) stand beside the step's 24 + 4 x n_terms B.
usage: dit_inpaint_step.py [--images 64] [--reps 200] [--warmup 20] [--windows 5] [--out FILE]  (GPU box)"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from naturaldiffusion_amd import ValidateNaturalInference as V  # noqa: E402
from naturaldiffusion_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from naturaldiffusion_amd.coeff import load_coeff_npz  # noqa: E402
from naturaldiffusion_amd.sampler import KNOWN_COLUMN0, ValidateNI, known_schedule  # noqa: E402

S = 32
SE = 4 * S * S
MATRIX = "results/ddpm/ddpm_024.npz"
ROWS = (1, 22)
SEED = 888


def left_half_mask(n_img, fraction, dev):
    m = torch.zeros((n_img, 4, S, S), dtype=torch.uint8)
    if fraction == 1.0:
        m[:] = 1
    elif fraction == 0.5:
        m[..., :S // 2] = 1
    return m.reshape(-1).to(dev)


def window(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                        # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n_img = args.images
    E = n_img * SE
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    z, noise, known, z_next = rnd(E), rnd(E), rnd(E), torch.empty(E, device=dev)
    cond, uncond = rnd(n_img, 2 * SE), rnd(n_img, 2 * SE)
    cfg = torch.full((n_img,), 4.0, device=dev)
    slots = torch.arange(n_img, dtype=torch.int32, device=dev)
    masks = {f: left_half_mask(n_img, f, dev) for f in (0.0, 0.5, 1.0)}
    C, B, node = load_coeff_npz(ROOT / MATRIX)
    tables, _ = V.skip_ddim_coeff(V.create_ddim_coeff(), B.shape[0])
    c1, c2 = np.asarray(tables[2])[::-1].astype(np.float32), np.asarray(tables[3])[::-1].astype(np.float32)
    ni = ValidateNI(C, B, node, c1, c2, E, device=dev, seed=SEED, elems_per_image=SE)
    ni.hist_x0.normal_(generator=g)                               # every history row the step reads holds finite data
    levels = known_schedule(node, "mean")
    torch.cuda.synchronize()
    results = []
    for k in ROWS:
        ic, vc, nc = ni.rows_c.ptrs(k)
        ib, vb, nb = ni.rows_b.ptrs(k)
        head = (ptr(z), ptr(cond), ptr(uncond), ptr(cfg), ptr(slots), n_img, SE, 2 * SE, ptr(ni.hist_x0), ptr(noise), ptr(z_next), ic, vc, nc,
                ni.rows_c.rows[k].diag, ib, vb, nb, k, ni.c1[k], ni.c2[k], SEED, None, 0, 1, E)
        alpha, std, _ = levels[k + 1]                             # the level the step's output is at (both rows: std > 0)
        variants = {"baseline": lambda: check(lib.natinf_step_f32prod_noise_guided(*head, stream_ptr()), "natinf_step_f32prod_noise_guided")}
        for f, m in masks.items():
            for name, s in (("draw", std), ("nodraw", 0.0)):
                variants[f"mask{f:g}_{name}"] = (lambda m=m, s=s: check(lib.natinf_step_f32prod_inpaint(
                    *head, ptr(known), ptr(m), SE, SE, alpha, s, KNOWN_COLUMN0 + k + 1, stream_ptr()), "natinf_step_f32prod_inpaint"))
        times = {v: [] for v in variants}
        for _ in range(args.windows):                             # alternate: every variant sees the same drift of the box
            for v, fn in variants.items():
                times[v].append(window(fn, args.reps, args.warmup))
        base = statistics.median(times["baseline"])
        row = dict(matrix=MATRIX, row=k, history_rows_read=nc, noise_terms=nb, step_bytes_per_element=24 + 4 * nc, blend_bytes_per_element=5,
                   level_alpha=alpha, level_std=std, us={})
        for v, ts in times.items():
            med = statistics.median(ts)
            row["us"][v] = dict(median=round(med, 2), min=round(min(ts), 2), max=round(max(ts), 2), against_baseline=round(med / base, 3))
            print(f"{MATRIX} row {k}: {v:14s} {med:8.2f} us (min {min(ts):.2f}, max {max(ts):.2f}) = {med / base:.3f} x baseline", flush=True)
        results.append(row)
    summary = dict(images=n_img, elems=E, reps=args.reps, warmup=args.warmup, windows=args.windows,
                   device=torch.cuda.get_device_name(dev), rows=results)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
