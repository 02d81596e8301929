"""Time of the step with the x0 projection (natinf_step_f64hist_project, one workgroup per image, at s = 2, 4 and 8) beside
natinf_step_f64hist_noise, the streaming baseline, and natinf_step_f64hist_x0fix in CLIP mode, the same kernel shape without a spatial pass, at
E = 512 x 3072 on row 14 of weights/step_15_weight_173.npz -- as a job runs it (the row's non-zero terms) and dense (all 14 history rows and the
diagonal) -- and beside one NCSN++ forward at the same batch, all in one process.
The steps: `windows` windows per variant, alternating variant by variant, each a HIP-event pair around `reps` back-to-back launches after
`warmup` launches; the median window is reported with the min and max.  The forward: the same with `forward_reps` forwards per window.
The condition (taken from 3i): the projection launch at every scale stays under 1 % of the forward measured in the same run.
usage: x0_project_step.py [--images 512] [--reps 200] [--warmup 20] [--windows 5] [--out profiles/x0_project/step_times.json]  (GPU box)"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from naturaldiffusion_amd._lib import X0_CLIP, check, lib, ptr, stream_ptr  # noqa: E402
from naturaldiffusion_amd.coeff import load_coeff_npz  # noqa: E402
from naturaldiffusion_amd.sampler import CifarNI  # noqa: E402

SHAPE = (3, 32, 32)
EPI = 3 * 32 * 32
MATRIX, ROW = "weights/step_15_weight_173.npz", 14
SCALES = (2, 4, 8)


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


def stats(ts):
    return dict(median=round(statistics.median(ts), 2), min=round(min(ts), 2), max=round(max(ts), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--forward-reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles/x0_project/step_times.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n_img, E, k = args.images, args.images * EPI, ROW
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda: torch.randn(E, device=dev, generator=g)
    x, out, noise, x_next = rnd(), rnd(), rnd(), torch.empty(E, device=dev)
    s_out = torch.empty(n_img, dtype=torch.float64, device=dev)
    r_out = torch.empty(n_img, dtype=torch.float64, device=dev)
    lows = {s: (torch.rand(n_img * EPI // (s * s), device=dev, generator=g, dtype=torch.float64) * 2 - 1) for s in SCALES}      # one picture per image
    C, B, node = load_coeff_npz(ROOT / MATRIX)
    summary = dict(images=n_img, elems=E, matrix=MATRIX, row=k, reps=args.reps, warmup=args.warmup, windows=args.windows,
                   device=torch.cuda.get_device_name(dev), steps=[])
    for dense in (False, True):
        ni = CifarNI(C, B, node, E, device=dev, seed=888, elems_per_image=EPI, dense=dense)
        ni.hist.normal_(generator=g)                              # every history row the step reads holds finite data
        idx, val, n = ni.rows.ptrs(k)
        ib, vb, nb = ni._noise_rows().ptrs(k)
        head = (ptr(x), ptr(out), ptr(noise), ptr(ni.hist), ptr(x_next), idx, val, n, ni.rows.rows[k].diag, ib, vb, nb, k,
                float(node[k, 1]), float(node[k, 2]), ni.std[k], 888, None, 0, 1, EPI, E)
        project = lambda s: (lambda: check(lib.natinf_step_f64hist_project(*head, ptr(lows[s]), EPI // (s * s), *SHAPE, s, ptr(r_out), stream_ptr()),
                                           "natinf_step_f64hist_project"))
        variants = {"noise_baseline": lambda: check(lib.natinf_step_f64hist_noise(*head, stream_ptr()), "natinf_step_f64hist_noise"),
                    "x0fix_clip": lambda: check(lib.natinf_step_f64hist_x0fix(*head, None, None, 0, 0, 0.0, 0.0, 0, X0_CLIP, 0.995, 1.0, ptr(s_out),
                                                                              stream_ptr()), "natinf_step_f64hist_x0fix")}
        variants.update({f"project_s{s}": project(s) for s in SCALES})
        times = {v: [] for v in variants}
        for _ in range(args.windows):                             # alternate: every variant sees the same drift of the box
            for v, fn in variants.items():
                times[v].append(window(fn, args.reps, args.warmup))
        torch.cuda.synchronize()
        row = dict(dense=dense, history_rows_read=n, noise_terms=nb, step_bytes_per_element=24 + 8 * n, us={v: stats(ts) for v, ts in times.items()})
        for v, st in row["us"].items():
            print(f"row {k} dense={dense}: {v:16s} {st['median']:8.2f} us (min {st['min']:.2f}, max {st['max']:.2f})", flush=True)
        summary["steps"].append(row)

    from naturaldiffusion_amd.ncsnpp import NCSNppEngine, flatten_state_dict
    from naturaldiffusion_amd.synth import synthetic_state_dict
    eng = NCSNppEngine(flatten_state_dict(synthetic_state_dict(0)), max_batch=n_img, device=dev)
    xin = torch.randn(n_img, 3, 32, 32, device=dev, generator=g)
    labels = torch.full((n_img,), float(node[k, 0]) * 999.0, device=dev)
    fwd = [window(lambda: eng(xin, labels), args.forward_reps, 2) for _ in range(args.windows)]
    summary["forward_us"] = stats(fwd)
    fmed = summary["forward_us"]["median"]
    print(f"NCSN++ forward at B = {n_img}: {fmed:.1f} us", flush=True)
    for row in summary["steps"]:
        row["share_of_forward_percent"] = {v: round(100.0 * st["median"] / fmed, 4) for v, st in row["us"].items()}
    shares = {f"project_s{s}": max(row["share_of_forward_percent"][f"project_s{s}"] for row in summary["steps"]) for s in SCALES}
    worst = max(shares.values())
    summary["condition"] = dict(text="project_s2 / s4 / s8 median < 1 % of the forward median of this run", worst_percent_by_scale=shares,
                                worst_percent=worst, met=bool(worst < 1.0))
    print(f"projection launch: {worst:.4f} % of the forward at worst ({shares}) -> condition {'met' if worst < 1.0 else 'NOT met'}", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
