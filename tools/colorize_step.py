"""Time of the colorization step (natinf_step_f64hist_colorize: natinf_step_f64hist_noise on the three planes of a pixel quad plus the
gray-channel blend in registers) beside natinf_step_f64hist_noise itself, the baseline, at E = 512 x 3072 on the last row of
weights/step_15_weight_173.npz (row 14: 14 history rows and the diagonal, a one-term noise row) and of results/euler_heun/sde_euler_024.npz
(row 23: a stochastic row).  The blend once with a draw (std of the row's own level) and once without (std 0, what the last step of a job does).
Both entries run in one process: `windows` windows per variant, alternating variant by variant, each a HIP-event pair around `reps` back-to-back
launches after `warmup` launches; the median window is reported with the min and max.  The 4 B per pixel the blend adds (gray_u: 4/3 B per
element) stand beside the step's 24 + 8 x n_terms B per element.
usage: colorize_step.py [--images 512] [--reps 200] [--warmup 20] [--windows 5] [--out FILE]  (GPU box)"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from naturaldiffusion_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from naturaldiffusion_amd.coeff import load_coeff_npz  # noqa: E402
from naturaldiffusion_amd.sampler import COLOR_COLUMN0, COLOR_M, COLOR_W, CifarNI  # noqa: E402

EPI = 3 * 32 * 32
ROWS = (("weights/step_15_weight_173.npz", 14), ("results/euler_heun/sde_euler_024.npz", 23))


def window(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                        # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    E = args.images * EPI
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda n=E: torch.randn(n, device=dev, generator=g)
    x, out, noise, gray, x_next = rnd(), rnd(), rnd(), rnd(E // 3), torch.empty(E, device=dev)
    f9 = lambda m: (ctypes.c_float * 9)(*np.asarray(m, np.float32).reshape(-1).tolist())
    M, W = f9(COLOR_M), f9(COLOR_W)
    results = []
    for rel, k in ROWS:
        C, B, node = load_coeff_npz(ROOT / rel)
        ni = CifarNI(C, B, node, E, device=dev, seed=888, elems_per_image=EPI)
        ni.hist.normal_(generator=g)                              # every history row the step reads holds finite data
        idx, val, n = ni.rows.ptrs(k)
        ib, vb, nb = ni._noise_rows().ptrs(k)
        head = (ptr(x), ptr(out), ptr(noise), ptr(ni.hist), ptr(x_next), idx, val, n, ni.rows.rows[k].diag, ib, vb, nb, k,
                float(node[k, 1]), float(node[k, 2]), ni.std[k], 888, None, 0, 1, EPI, E)
        alpha, std = float(np.float32(node[k, 1])), float(np.float32(node[k, 2]))
        variants = {"baseline": lambda: check(lib.natinf_step_f64hist_noise(*head, stream_ptr()), "natinf_step_f64hist_noise")}
        for name, s in (("draw", std), ("nodraw", 0.0)):
            variants[f"colorize_{name}"] = (lambda s=s: check(lib.natinf_step_f64hist_colorize(
                *head, ptr(gray), EPI // 3, M, W, alpha, s, COLOR_COLUMN0 + k, stream_ptr()), "natinf_step_f64hist_colorize"))
        times = {v: [] for v in variants}
        for _ in range(args.windows):                             # alternate: every variant sees the same drift of the box
            for v, fn in variants.items():
                times[v].append(window(fn, args.reps, args.warmup))
        base = statistics.median(times["baseline"])
        row = dict(matrix=rel, row=k, history_rows_read=n, noise_terms=nb, step_bytes_per_element=24 + 8 * n,
                   blend_bytes_per_element=round(4 / 3, 3), level_alpha=alpha, level_std=std, us={})
        for v, ts in times.items():
            med = statistics.median(ts)
            row["us"][v] = dict(median=round(med, 2), min=round(min(ts), 2), max=round(max(ts), 2), against_baseline=round(med / base, 3))
            print(f"{rel} row {k}: {v:16s} {med:8.2f} us (min {min(ts):.2f}, max {max(ts):.2f}) = {med / base:.3f} x baseline", flush=True)
        results.append(row)
    summary = dict(images=args.images, elems=E, reps=args.reps, warmup=args.warmup, windows=args.windows,
                   device=torch.cuda.get_device_name(dev), rows=results)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
