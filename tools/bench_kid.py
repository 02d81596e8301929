"""Time and error of the Kernel Inception Distance (naturaldiffusion_amd/kid.py: planes of both sets, three kernel-sum sweeps, the host reduction) beside the
plain torch statements on the same device, in the same process, on the same inputs: ((a @ b.T) * gamma + coef0) ** 3 in fp32, CHUNK rows at a time, summed.
usage: bench_kid.py [--out FILE] [n:d ...]        (default: 10000:2048 50000:2048 -- real and generated sets of n rows each, gamma = 1 / d, coef0 = 1)
Both estimators run: "full" (the whole sets) and "blocks" (TF-GAN's, max_block_size 1024).  Inputs are cluster features generated on the device
(tests/prdc_oracle.py's recipe).  The protocol is tools/bench_prdc.py's: times are host clocks around device-synchronised work on device-resident inputs; all
four jobs are first run at the FULL shape (allocator blocks, code objects and the BLAS library's choice for every GEMM shape are then in place); then REPEATS
windows of each job alternate (kernels full, torch full, kernels blocks, torch blocks, kernels full, ...), every window holding as many whole jobs as make about
WINDOW_S seconds, and the median, the smallest and the largest time per job are reported.  The sweeps' own times are medians of REPEATS device-event timings,
beside one knn_radii pass (prdc.py) of the same shape from the same run.  The error is taken against fp64 on the device: the largest relative error of the
real x generated row sums on a sample of SAMPLE rows, and the absolute error of the full estimate on the first SUBSET rows of both sets.  Prints one JSON object
per shape (and writes the list to FILE)."""
import json, math, statistics, sys, time
from pathlib import Path
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CHUNK = 2048          # rows per torch statement: a 2048 x 50000 fp32 kernel block is 0.4 GB
SAMPLE = 256
SUBSET = 4096
MAX_BLOCK = 1024
REPEATS = 7
WINDOW_S = 0.5        # seconds of work per timed window, at least one whole job


def cluster_feats(n, d, shift, seed, dev):
    W = torch.randn(6, d, generator=torch.Generator(device=dev).manual_seed(1234), device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, d, generator=g, device=dev).mul_(0.3)
    x.addmm_(torch.randn(n, 6, generator=g, device=dev) + shift, W).relu_().mul_(0.5)
    return x


def torch_row_sums(a, b, gamma, coef0, own=False, chunk=CHUNK):
    """the statement (fp32, or fp64: the dtype is the inputs'), one row sum per row of a; `own`: a is b, the diagonal is taken off"""
    out = torch.empty(a.shape[0], dtype=a.dtype, device=a.device)
    for s in range(0, a.shape[0], chunk):
        k = ((a[s:s + chunk] @ b.t()) * gamma + coef0) ** 3
        out[s:s + chunk] = k.sum(1) - (k.diagonal(s) if own else 0.0)
    return out


def mmd2(sxx, m, syy, n, sxy):
    return sxx / (m * (m - 1)) + syy / (n * (n - 1)) - 2.0 * sxy / (m * n)


def torch_full(real, gen, gamma, coef0):
    tot = lambda v: float(v.double().sum())
    return mmd2(tot(torch_row_sums(real, real, gamma, coef0, True)), real.shape[0], tot(torch_row_sums(gen, gen, gamma, coef0, True)), gen.shape[0],
                tot(torch_row_sums(real, gen, gamma, coef0)))


def torch_blocks(real, gen, gamma, coef0, bounds):
    est = [torch_full(real[r.start:r.stop], gen[g.start:g.stop], gamma, coef0) for r, g in zip(*bounds)]
    mean = math.fsum(est) / len(est)
    var = math.fsum((e - mean) ** 2 for e in est) / (len(est) - 1) if len(est) > 1 else 0.0
    return mean, math.sqrt(var / len(est))


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
    from naturaldiffusion_amd import kid as K
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
        gamma, coef0 = 1.0 / d, 1.0
        bounds = K.block_bounds(n, n, MAX_BLOCK)
        jobs = dict(kernels_full=lambda: K.kid(P.FeatureSet(real), P.FeatureSet(gen), estimator="full", group=K.LOCAL),
                    torch_full=lambda: torch_full(real, gen, gamma, coef0),
                    kernels_blocks=lambda: K.kid(P.FeatureSet(real), P.FeatureSet(gen), estimator="blocks", max_block_size=MAX_BLOCK, group=K.LOCAL),
                    torch_blocks=lambda: torch_blocks(real, gen, gamma, coef0, bounds))
        # warm-up of every job at the full shape; the second run's time only sizes the windows
        values, iters = {}, {}
        for name, fn in jobs.items():
            values[name] = wall(fn)[0]
        for name, fn in jobs.items():
            iters[name] = max(1, round(WINDOW_S / wall(fn)[1]))
        ts = {name: [] for name in jobs}
        for _ in range(REPEATS):                                                        # the jobs alternate
            for name, fn in jobs.items():
                ts[name].append(wall(fn, iters[name])[1])
        med = {name: statistics.median(v) for name, v in ts.items()}
        fr, fg = P.FeatureSet(real), P.FeatureSet(gen)
        med_ms = lambda fn: round(statistics.median(event_ms(fn)[1] for _ in range(REPEATS)), 3)
        P.knn_radii(fr, 3)
        sweeps = dict(planes_both=med_ms(lambda: (P.FeatureSet(real), P.FeatureSet(gen))),
                      real_x_real=med_ms(lambda: K.kernel_row_sums(fr, range(n), fr, exclude_self=True)),
                      gen_x_gen=med_ms(lambda: K.kernel_row_sums(fg, range(n), fg, exclude_self=True)),
                      real_x_gen=med_ms(lambda: K.kernel_row_sums(fr, range(n), fg)),
                      knn_radii_one_set=med_ms(lambda: P.knn_radii(fr, 3)))
        # the error of the row sums on a row sample, fp64 on the device
        rows = range(n // 3, n // 3 + min(SAMPLE, n))
        ref = torch_row_sums(real[rows.start:rows.stop].double(), gen.double(), gamma, coef0, chunk=64)
        rel = lambda v: float(((v.double() - ref) / ref).abs().max())
        err_rows = dict(kernels=rel(K.kernel_row_sums(fr, rows, fg)), torch=rel(torch_row_sums(real[rows.start:rows.stop], gen, gamma, coef0)))
        # ... and of the full estimate on a subset
        m = min(SUBSET, n)
        rs, gs = real[:m].contiguous(), gen[:m].contiguous()
        kid64 = torch_full(rs.double(), gs.double(), gamma, coef0)
        kid_k, kid_t = K.kid(rs, gs, estimator="full", group=K.LOCAL)["kid"], torch_full(rs, gs, gamma, coef0)
        flop = 3 * 2.0 * n * n * d
        res = dict(n=n, d=d, max_block_size=MAX_BLOCK, n_blocks=len(bounds[0]), seconds={name: spread(v) for name, v in ts.items()},
                   speedup_of_medians=dict(full=round(med["torch_full"] / med["kernels_full"], 3), blocks=round(med["torch_blocks"] / med["kernels_blocks"], 3)),
                   repeats=REPEATS, jobs_per_window=iters, kernels_ms=sweeps,
                   full_tflops_fp32_equivalent=round(flop / med["kernels_full"] / 1e12, 1),
                   row_sum_rel_err=err_rows, sample_rows=len(rows),
                   subset_rows=m, subset_kid_fp64=kid64, subset_kid_abs_err=dict(kernels=abs(kid_k - kid64), torch=abs(kid_t - kid64)),
                   kid=dict(kernels_full=values["kernels_full"]["kid"], torch_full=values["torch_full"],
                            kernels_blocks=[values["kernels_blocks"]["kid"], values["kernels_blocks"]["std"]], torch_blocks=list(values["torch_blocks"])))
        print(json.dumps(res), flush=True)
        results.append(res)
        del real, gen, fr, fg, rs, gs, jobs
        torch.cuda.empty_cache()
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
