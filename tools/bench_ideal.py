"""Time, peak memory and error of the ideal denoiser (naturaldiffusion_amd/ideal.py: the distance sweep, the row softmax, the weighted sum over K ranges,
the merge) beside the plain torch statements ``softmax(-c * cdist(u, F)**2) @ F`` in fp32 on the same device, in the same process, on the same inputs.
usage: bench_ideal.py [--out FILE] [--label TEXT] [--kernels-only] [B:N:d ...]        (default: 256:50000:3072 64:50000:3072)
The training set is synthetic uint8 pictures (tools/bench_nn.py's recipe) centred to [-1, 1]; the queries are training rows noised to a VP level,
x_t = alpha f + sigma eps, at a low-noise (t = 0.05), a mid-noise (t = 0.4) and a high-noise (t = 0.8) level, u = x_t / alpha and c = alpha^2 / (2 sigma^2).  Times are host clocks
around device-synchronised work on device-resident inputs with the training set prepared: both sides are first run twice; then REPEATS windows of each side
alternate (kernels, torch, kernels, ...), every window holding as many whole calls as make about WINDOW_S seconds, and the median, the smallest and the largest
time per call are reported.  Peak memory is the allocator's high-water mark over one call, above what was allocated before it.  Error: max |x0 - ref| of
both sides on SAMPLE rows against an fp64 evaluation on the device.  ``ncsnpp_forward_ms`` is an NCSN++ forward (synthetic weights) of the same batch: what
the denoiser a sampling job usually pays for costs beside this one.  ``--kernels-only`` leaves the torch side, the error and the NCSN++ forward out (the sweep
over builds with other NATINF_IDEAL_K_RANGE / NATINF_IDEAL_CHUNK_ROWS, chosen with NATINF_LIB; ``--label`` names the build in the output).
Prints one JSON object per shape and level (and writes the list to FILE)."""
import json, statistics, sys
from pathlib import Path
import numpy as np
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from bench_prdc import event_ms, score_block, spread, wall
from bench_nn import peak_bytes, pixel_feats

SAMPLE = 64
REPEATS = 7
WINDOW_S = 0.5
LEVELS = (("low", 0.05), ("mid", 0.4), ("high", 0.8))


def main(argv):
    from naturaldiffusion_amd import ideal as I
    from naturaldiffusion_amd import _lib, coeffgen
    _lib.require_gpu()
    out_path, label, quick = None, "", False
    if "--out" in argv:
        i = argv.index("--out"); out_path = argv[i + 1]; del argv[i:i + 2]
    if "--label" in argv:
        i = argv.index("--label"); label = argv[i + 1]; del argv[i:i + 2]
    if "--kernels-only" in argv:
        argv.remove("--kernels-only"); quick = True
    shapes = [tuple(int(v) for v in a.split(":")) for a in argv] or [(256, 50000, 3072), (64, 50000, 3072)]
    dev = torch.device("cuda:0")
    results = []
    for B, N, d in shapes:
        F = ((pixel_feats(N, d, 1, dev).double() + 0.5) / 255.0 * 2.0 - 1.0).float()
        _, prep_ms = event_ms(lambda: I.TrainingSet(F))
        train = I.TrainingSet(F)
        g = torch.Generator(device=dev).manual_seed(7)
        own = torch.randint(0, N, (B,), generator=g, device=dev)
        eps = torch.randn(B, d, generator=g, device=dev)
        ncsn_ms = None
        if not quick and d == 3072:
            from naturaldiffusion_amd.ncsnpp import NCSNppEngine, flatten_state_dict
            from naturaldiffusion_amd.synth import synthetic_state_dict
            eng = NCSNppEngine(flatten_state_dict(synthetic_state_dict(0)), max_batch=B, device=dev)
            xin, lab = eps.view(B, 3, 32, 32).contiguous(), torch.full((B,), 500.0, device=dev)
            eng(xin, lab); eng(xin, lab)
            ncsn_ms = round(statistics.median(event_ms(lambda: eng(xin, lab))[1] for _ in range(REPEATS)), 3)
            del eng
        for name, t in LEVELS:
            alpha, sigma = (float(v) for v in coeffgen.vp_alpha_sigma(t))
            x = alpha * F[own] + sigma * eps
            u, c = I.level_scalars(x, alpha, sigma)
            c_t = torch.from_numpy(np.array(c)).to(dev)
            c32 = c_t.float()[:, None]

            def kernels():
                return I.posterior_mean(u, c_t, train, return_stats=True)

            def statements():
                return torch.softmax(-c32 * torch.cdist(u, F) ** 2, dim=1) @ F

            wall(kernels)
            (x0_k, st), peak_k = peak_bytes(kernels)
            _, w_k = wall(kernels)
            it_k = max(1, round(WINDOW_S / w_k))
            res = dict(label=label, B=B, N=N, d=d, level=name, t=t, c=float(c[0]), mean_pmax=float(st["pmax"].mean()),
                       own_share=float((st["nearest"] == own).double().mean()), prepare_training_set_ms=round(prep_ms, 3))
            if quick:
                ts_k = [wall(kernels, it_k)[1] for _ in range(REPEATS)]
                res.update(kernels_s=spread(ts_k), peak_bytes=dict(kernels=int(peak_k)))
            else:
                wall(statements)
                x0_t, peak_t = peak_bytes(statements)
                _, w_t = wall(statements)
                it_t = max(1, round(WINDOW_S / w_t))
                ts_k, ts_t = [], []
                for _ in range(REPEATS):                                                    # the two sides alternate
                    ts_k.append(wall(kernels, it_k)[1])
                    ts_t.append(wall(statements, it_t)[1])
                n_s = min(SAMPLE, B)
                ud, Fd = u[:n_s].double(), F.double()
                z = -c_t[:n_s, None] * score_block(ud, (ud * ud).sum(1), Fd, (Fd * Fd).sum(1)).clamp_min_(0.0)
                ref = torch.softmax(z, dim=1) @ Fd
                res.update(kernels_s=spread(ts_k), torch_s=spread(ts_t), torch_over_kernels_of_medians=round(statistics.median(ts_t) / statistics.median(ts_k), 3),
                           repeats=REPEATS, calls_per_window=dict(kernels=it_k, torch=it_t), peak_bytes=dict(kernels=int(peak_k), torch=int(peak_t)),
                           sample_rows=n_s, sample_max_abs_x0_error=dict(kernels=float((x0_k[:n_s].double() - ref).abs().max()),
                                                                         torch=float((x0_t[:n_s].double() - ref).abs().max())),
                           ncsnpp_forward_ms=ncsn_ms)
                del ud, Fd, z, ref, x0_t
            print(json.dumps(res), flush=True)
            results.append(res)
        del F, train
        torch.cuda.empty_cache()
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
