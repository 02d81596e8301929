"""Time, peak memory and exactness of the nearest-neighbour search (naturaldiffusion_amd/neighbours.py: planes of both sets, one sweep that keeps (distance,
index) pairs, the merge) beside ``torch.cdist`` + ``topk`` on the same device, in the same process, on the same inputs.
usage: bench_nn.py [--out FILE] [--k K] [n:d ...]        (default: 50000:2048 50000:3072 -- n generated rows against n reference columns, k = 1)
d = 3072 is pixel space: uint8-valued features (smooth low-rank pictures plus noise, rounded to 0..255, generated on the device), on which the sweep's
distances are exact integers; every other d is cluster features by tests/prdc_oracle.py's recipe.  Times are host clocks around device-synchronised work on
device-resident fp32 inputs.  Both sides are first run twice at the full shape; then REPEATS windows of each side alternate (kernels, torch, kernels, ...),
every window holding as many whole jobs as make about WINDOW_S seconds, and the median, the smallest and the largest time per job are reported.  The parts are
medians of REPEATS device-event timings; ``knn_radius_ms`` is natinf_prdc_knn_radius at the same shape: the same sweep without the indices.  Peak memory
is the allocator's high-water mark over one job, above what was allocated before it (the inputs).  Exactness: over all rows, how many of torch's nearest
indices differ from the kernels'; on SAMPLE rows, how many of either side's differ from an fp64 evaluation on the device, and whether the kernels' nearest
distance equals the fp64 one exactly.  Prints one JSON object per shape (and writes the list to FILE)."""
import json, statistics, sys
from pathlib import Path
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from bench_prdc import cluster_feats, event_ms, score_block, spread, wall

SAMPLE = 256
REPEATS = 7
WINDOW_S = 0.5        # seconds of work per timed window, at least one whole job
PIXEL_D = 3072


def pixel_feats(n, d, seed, dev):
    """uint8-valued fp32 [n, d]: twelve shared patterns mixed per image, plus noise"""
    W = torch.randn(12, d, generator=torch.Generator(device=dev).manual_seed(4321), device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, d, generator=g, device=dev).mul_(12.0)
    x.addmm_(torch.randn(n, 12, generator=g, device=dev), W, alpha=30.0).add_(128.0)
    return x.round_().clamp_(0.0, 255.0)


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def main(argv):
    from naturaldiffusion_amd import neighbours as N
    from naturaldiffusion_amd import prdc as P
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    out_path, k = None, 1
    if "--out" in argv:
        i = argv.index("--out"); out_path = argv[i + 1]; del argv[i:i + 2]
    if "--k" in argv:
        i = argv.index("--k"); k = int(argv[i + 1]); del argv[i:i + 2]
    shapes = [tuple(int(v) for v in a.split(":")) for a in argv] or [(50000, 2048), (50000, PIXEL_D)]
    dev = torch.device("cuda:0")
    results = []
    for n, d in shapes:
        pixels = d == PIXEL_D
        if pixels:
            cols, rows = pixel_feats(n, d, 1, dev), pixel_feats(n, d, 2, dev)
        else:
            cols, rows = cluster_feats(n, d, 0.0, 1, dev), cluster_feats(n, d, 0.6, 2, dev)

        def kernels():
            return N.nearest(P.FeatureSet(rows), P.FeatureSet(cols), k=k)

        def statements():
            v, i = torch.cdist(rows, cols).topk(k, dim=1, largest=False)
            return v * v, i

        # warm-up of both sides at the full shape, twice; the second run's time sizes the windows and its high-water mark is the reported peak
        wall(kernels); wall(statements)
        ((d2_k, idx_k), peak_k), ((d2_t, idx_t), peak_t) = peak_bytes(kernels), peak_bytes(statements)
        _, w_kernels = wall(kernels)
        _, w_torch = wall(statements)
        it_k, it_t = max(1, round(WINDOW_S / w_kernels)), max(1, round(WINDOW_S / w_torch))
        ts_k, ts_t = [], []
        for _ in range(REPEATS):                                                        # the two sides alternate
            ts_k.append(wall(kernels, it_k)[1])
            ts_t.append(wall(statements, it_t)[1])
        t_kernels, t_torch = statistics.median(ts_k), statistics.median(ts_t)
        med_ms = lambda fn: statistics.median(event_ms(fn)[1] for _ in range(REPEATS))
        fr, fc = P.FeatureSet(rows), P.FeatureSet(cols)
        ms_planes = med_ms(lambda: (P.FeatureSet(rows), P.FeatureSet(cols)))
        ms_nearest = med_ms(lambda: N.nearest(fr, fc, k=k))
        ms_radius = med_ms(lambda: P._knn(fr, range(n), fc, k, -1))
        del fr, fc
        # exactness on a row sample, fp64 on the device
        sl = slice(n // 3, n // 3 + min(SAMPLE, n))
        rd, cd = rows[sl].double(), cols.double()
        d2_64 = score_block(rd, (rd * rd).sum(1), cd, (cd * cd).sum(1))
        best_64, idx_64 = d2_64.min(1)
        res = dict(n=n, d=d, k=k, space="pixel" if pixels else "features", kernels_s=spread(ts_k), torch_s=spread(ts_t),
                   torch_over_kernels_of_medians=round(t_torch / t_kernels, 3), repeats=REPEATS, jobs_per_window=dict(kernels=it_k, torch=it_t),
                   kernels_ms=dict(planes_both=round(ms_planes, 3), nearest=round(ms_nearest, 3), knn_radius_ms=round(ms_radius, 3)),
                   peak_bytes=dict(kernels=int(peak_k), torch=int(peak_t)),
                   rows_where_torch_nearest_differs_from_kernels=int((idx_t[:, 0] != idx_k[:, 0]).sum()),
                   sample_rows=int(rd.shape[0]),
                   sample_nearest_differing_from_fp64=dict(kernels=int((idx_k[sl, 0] != idx_64).sum()), torch=int((idx_t[sl, 0] != idx_64).sum())),
                   sample_kernels_d2_equals_fp64=bool((d2_k[sl, 0] == best_64).all()),
                   sample_max_rel_d2_error=dict(kernels=float(((d2_k[sl, 0] - best_64).abs() / best_64).max()),
                                                torch=float(((d2_t[sl, 0].double() - best_64).abs() / best_64).max())))
        print(json.dumps(res), flush=True)
        results.append(res)
        del rows, cols, rd, cd, d2_64, d2_k, idx_k, d2_t, idx_t
        torch.cuda.empty_cache()
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
