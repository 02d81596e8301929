"""Time and error of the k-nearest-neighbour manifold metrics (naturaldiffusion_amd/prdc.py: planes, two radius passes, two ball-count passes) beside the plain
torch statements on the same device, in the same process, on the same inputs: chunked fp32 |a|^2 + |b|^2 - 2 a.b, kthvalue with the diagonal at +inf, compare.
usage: bench_prdc.py [--out FILE] [n:d ...]        (default: 10000:2048 50000:2048 -- real and generated sets of n rows each, k = 3)
Inputs are cluster features generated on the device (tests/prdc_oracle.py's recipe).  Times are host clocks around device-synchronised work on
device-resident inputs.  Both sides are first run once at the FULL shape (every chunk, the tail chunk included: allocator blocks, code objects and the BLAS
library's choice for every GEMM shape are then in place); then REPEATS windows of each side alternate (kernels, torch, kernels, ...), every window holding as
many whole jobs as make about WINDOW_S seconds, and the median, the smallest and the largest time per job are reported.  The kernels' parts are the medians of
REPEATS device-event timings.  The error is taken on a
sample of 256 real rows against an fp64 evaluation on the device: the largest |r2 - r2_fp64| / (|a_i|^2 + max_j |b_j|^2) of the radii, and the number of
sampled rows whose coverage / recall counts differ from the fp64 counts.  Prints one JSON object per shape (and writes the list to FILE)."""
import json, statistics, sys, time
from pathlib import Path
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

K = 3
CHUNK = 2048          # rows per torch statement: a 2048 x 50000 fp32 score block is 0.4 GB
SAMPLE = 256
REPEATS = 7
WINDOW_S = 0.5        # seconds of work per timed window, at least one whole job


def cluster_feats(n, d, shift, seed, dev):
    W = torch.randn(6, d, generator=torch.Generator(device=dev).manual_seed(1234), device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, d, generator=g, device=dev).mul_(0.3)
    x.addmm_(torch.randn(n, 6, generator=g, device=dev) + shift, W).relu_().mul_(0.5)
    return x


def score_block(a, na, b, nb):
    """the fp32 statement (also the fp64 one: the dtype is the inputs')"""
    return na[:, None] + nb[None, :] - 2.0 * (a @ b.t())


def torch_radii(x, nx, k, rows=None, chunk=CHUNK):
    rows = range(x.shape[0]) if rows is None else rows
    out = torch.empty(len(rows), dtype=x.dtype, device=x.device)
    for s in range(rows.start, rows.stop, chunk):
        e = min(s + chunk, rows.stop)
        d2 = score_block(x[s:e], nx[s:e], x, nx)
        i = torch.arange(e - s, device=x.device)
        d2[i, i + s] = float("inf")
        out[s - rows.start:e - rows.start] = d2.kthvalue(k, dim=1).values
    return out


def torch_statements(real, gen, k):
    """the four count vectors with plain torch in fp32"""
    nr, ng = (real * real).sum(1), (gen * gen).sum(1)
    r2_real, r2_gen = torch_radii(real, nr, k), torch_radii(gen, ng, k)
    g_in_r = torch.empty(gen.shape[0], dtype=torch.int64, device=gen.device)
    for s in range(0, gen.shape[0], CHUNK):
        g_in_r[s:s + CHUNK] = (score_block(gen[s:s + CHUNK], ng[s:s + CHUNK], real, nr) <= r2_real[None, :]).sum(1)
    r_in_g, own = torch.empty(real.shape[0], dtype=torch.int64, device=gen.device), torch.empty(real.shape[0], dtype=torch.int64, device=gen.device)
    for s in range(0, real.shape[0], CHUNK):
        d2 = score_block(real[s:s + CHUNK], nr[s:s + CHUNK], gen, ng)
        r_in_g[s:s + CHUNK] = (d2 <= r2_gen[None, :]).sum(1)
        own[s:s + CHUNK] = (d2 <= r2_real[s:s + CHUNK, None]).sum(1)
    return dict(r2_real=r2_real, r2_gen=r2_gen, gen_in_real_balls=g_in_r, real_in_gen_balls=r_in_g, gen_in_own_ball=own)


def wall(fn, iters=1):
    """(last result, seconds per call) of `iters` calls in one device-synchronised window"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) / iters


def spread(ts, digits=5):
    return dict(median=round(statistics.median(ts), digits), min=round(min(ts), digits), max=round(max(ts), digits))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record(); b.synchronize()
    return out, a.elapsed_time(b)


def main(argv):
    from naturaldiffusion_amd import prdc as P
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    out_path = None
    if "--out" in argv:
        i = argv.index("--out"); out_path = argv[i + 1]; del argv[i:i + 2]
    shapes = [tuple(int(v) for v in a.split(":")) for a in argv] or [(10000, 2048), (50000, 2048)]
    dev = torch.device("cuda:0")
    results = []
    for n, d in shapes:
        real, gen = cluster_feats(n, d, 0.0, 1, dev), cluster_feats(n, d, 0.6, 2, dev)

        def kernels():
            fr, fg = P.FeatureSet(real), P.FeatureSet(gen)
            c = P.prdc_counts(fr, fg, K)
            return fr, fg, c, P.prdc_from_sums(P.count_sums(c), K)

        statements = lambda: torch_statements(real, gen, K)
        # warm-up of both sides at the full shape; its times only size the windows
        (fr, fg, counts, numbers), w_kernels = wall(kernels)
        ref, w_torch = wall(statements)
        _, w_kernels = wall(kernels)
        _, w_torch = wall(statements)
        it_k, it_t = max(1, round(WINDOW_S / w_kernels)), max(1, round(WINDOW_S / w_torch))
        ts_k, ts_t = [], []
        for _ in range(REPEATS):                                                        # the two sides alternate
            ts_k.append(wall(kernels, it_k)[1])
            ts_t.append(wall(statements, it_t)[1])
        t_kernels, t_torch = statistics.median(ts_k), statistics.median(ts_t)
        med_ms = lambda fn: statistics.median(event_ms(fn)[1] for _ in range(REPEATS))
        ms_planes = med_ms(lambda: (P.FeatureSet(real), P.FeatureSet(gen)))
        r2_real, r2_gen = P.knn_radii(fr, K), P.knn_radii(fg, K)
        ms_knn = med_ms(lambda: P.knn_radii(fr, K))
        ms_balls = med_ms(lambda: P._balls(fr, range(n), fg, r2_real, r2_gen))
        # the error on a row sample, fp64 on the device
        rows = range(n // 3, n // 3 + min(SAMPLE, n))
        rd, gd = real.double(), gen.double()
        nr64, ng64 = (rd * rd).sum(1), (gd * gd).sum(1)
        r2_64 = torch_radii(rd, nr64, K, rows, chunk=64)
        r2_gen_64 = torch_radii(gd, ng64, K, chunk=512)
        d2 = score_block(rd[rows.start:rows.stop], nr64[rows.start:rows.stop], gd, ng64)
        own_64, rin_64 = (d2 <= r2_64[:, None]).sum(1), (d2 <= r2_gen_64[None, :]).sum(1)
        scale = nr64[rows.start:rows.stop] + nr64.max()
        sl = slice(rows.start, rows.stop)
        err = lambda r2: float(((r2[sl].double() - r2_64).abs() / scale).max())
        diff = lambda c: [int((c["gen_in_own_ball"][sl].long() != own_64).sum()), int((c["real_in_gen_balls"][sl].long() != rin_64).sum())]
        flop = 4 * 2.0 * n * n * d
        res = dict(n=n, d=d, k=K, kernels_s=spread(ts_k), torch_s=spread(ts_t), speedup_of_medians=round(t_torch / t_kernels, 3),
                   repeats=REPEATS, jobs_per_window=dict(kernels=it_k, torch=it_t),
                   kernels_ms=dict(planes_both=round(ms_planes, 3), knn_one_set=round(ms_knn, 3), balls_both_counts=round(ms_balls, 3)),
                   distance_tflops_fp32_equivalent=round(flop / t_kernels / 1e12, 1),
                   radius_err_kernels=err(r2_real), radius_err_torch=err(ref["r2_real"]),
                   sample_rows=len(rows), count_rows_differing_kernels=diff(counts), count_rows_differing_torch=diff(ref),
                   numbers=numbers)
        print(json.dumps(res), flush=True)
        results.append(res)
        del real, gen, fr, fg, rd, gd
        torch.cuda.empty_cache()
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
