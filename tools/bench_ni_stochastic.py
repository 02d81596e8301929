"""Per-step time of the stochastic CIFAR10 step (k_step_noise_f64: signal sum over the fp64 history + the noise row, eps_j for j >= 1
generated in registers by Philox) on every step of results/euler_heun/sde_euler_024.npz at B = 512 images, beside k_step_f64hist on the
same C row with column 0 of B only.  HIP events around `reps` back-to-back launches of one step after `warmup` launches; prints one line
per step (us per launch, history GB/s = fp64 history bytes read and written over the launch time) and a JSON summary.
usage: bench_ni_stochastic.py [--images 512] [--reps 200] [--warmup 20] [--out FILE]  (GPU box)"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from naturaldiffusion_amd.coeff import load_coeff_npz  # noqa: E402
from naturaldiffusion_amd.sampler import CifarNI  # noqa: E402


def time_step(ni, k, x, out, noise, x_next, reps, warmup, **kw):
    for _ in range(warmup):
        ni.step(k, x, out, noise, x_next=x_next, **kw)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        ni.step(k, x, out, noise, x_next=x_next, **kw)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                       # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    C, B, node = load_coeff_npz(ROOT / "results/euler_heun/sde_euler_024.npz")
    n, epi = C.shape[0], 3 * 32 * 32
    E = args.images * epi
    B0 = B.copy()
    B0[:, 1:] = 0.0                                              # the same matrix with column 0 only -> k_step_f64hist
    sto = CifarNI(C, B, node, E, device=dev, seed=888, elems_per_image=epi)
    det = CifarNI(C, B0, node, E, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    noise = torch.randn(E, device=dev, generator=g)
    outs = [torch.randn(E, device=dev, generator=g) for _ in range(n)]
    x_next = torch.empty(E, device=dev)
    for ni, kw in ((sto, dict(index=0)), (det, {})):             # fill every history slot once
        x = noise
        for k in range(n):
            x = ni.step(k, x, outs[k], noise, **kw)
    torch.cuda.synchronize()
    rows = []
    for k in range(n):
        nt = sto.rows.rows[k].n
        hist_bytes = (nt + 1) * E * 8                            # n_terms rows read + slot k written, fp64
        io_bytes = 3 * E * 4                                     # x_k, model_out, x_next (fp32); + noise when column 0 is read
        t_sto = time_step(sto, k, noise, outs[k], noise, x_next, args.reps, args.warmup, index=0)
        t_det = time_step(det, k, noise, outs[k], noise, x_next, args.reps, args.warmup)
        r = dict(step=k, c_terms=nt + 1, b_terms=sto.rows_b.rows[k].n, us_stochastic=round(t_sto, 2), us_column0=round(t_det, 2),
                 hist_GBps_stochastic=round(hist_bytes / t_sto / 1e3, 1), hist_GBps_column0=round(hist_bytes / t_det / 1e3, 1),
                 all_GBps_column0=round((hist_bytes + io_bytes + E * 4) / t_det / 1e3, 1))
        rows.append(r)
        print(f"step {k:2d}: C terms {r['c_terms']:2d}, B terms {r['b_terms']:2d}: stochastic {t_sto:7.1f} us ({r['hist_GBps_stochastic']:6.0f} GB/s history), "
              f"column 0 only {t_det:7.1f} us ({r['hist_GBps_column0']:6.0f} GB/s history)", flush=True)
    tot_s, tot_d = sum(r["us_stochastic"] for r in rows), sum(r["us_column0"] for r in rows)
    summary = dict(matrix="results/euler_heun/sde_euler_024.npz", images=args.images, elems=E, reps=args.reps, warmup=args.warmup,
                   total_ms_stochastic=round(tot_s / 1e3, 3), total_ms_column0=round(tot_d / 1e3, 3),
                   device=torch.cuda.get_device_name(dev), steps=rows)
    print(json.dumps({k: v for k, v in summary.items() if k != "steps"}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
