"""Time and error of the Inception Score (naturaldiffusion_amd/iscore.py: planes of the features, the logit sweep against the head, the row statistics, the
host reduction) beside the plain torch statements on the same device, in the same process, on the same inputs: log_softmax(feats @ W.T + b) in fp32, the
rows' negative entropy, the mean marginal.
usage: bench_is.py [--out FILE] [n:classes:d ...]        (default: 50000:1008:2048)
Inputs are cluster features generated on the device (tests/prdc_oracle.py's recipe) and synth.synthetic_inception_head.  The protocol is tools/bench_kid.py's:
times are host clocks around device-synchronised work on device-resident inputs; both jobs are first run at the full shape; then REPEATS windows of each job
alternate (kernels, torch, kernels, ...), every window holding as many whole jobs as make about WINDOW_S seconds, and the median, the smallest and the largest
time per job are reported.  The parts' own times are medians of REPEATS device-event timings.  The error is taken against fp64 on the device on the first
SUBSET rows: the absolute error of log IS and the largest absolute errors of the rows' negative entropy and log-sum-exp.  Prints one JSON object per shape
(and writes the list to FILE)."""
import json, statistics, sys, time
from pathlib import Path
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SUBSET = 2000
REPEATS = 7
WINDOW_S = 0.5        # seconds of work per timed window, at least one whole job


def cluster_feats(n, d, shift, seed, dev):
    W = torch.randn(6, d, generator=torch.Generator(device=dev).manual_seed(1234), device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, d, generator=g, device=dev).mul_(0.3)
    x.addmm_(torch.randn(n, 6, generator=g, device=dev) + shift, W).relu_().mul_(0.5)
    return x


def torch_stats(x, W, b):
    """(h [n], lse [n], log IS) by the statements, in the dtype of the inputs"""
    z = x @ W.t() + b
    lp = torch.log_softmax(z, 1)
    p = lp.exp()
    h = (p * lp).sum(1)
    pbar = p.mean(0)
    nz = pbar > 0
    return h, torch.logsumexp(z, 1), float(h.mean() - (pbar[nz] * pbar[nz].log()).sum())


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
    from naturaldiffusion_amd import iscore as I
    from naturaldiffusion_amd import prdc as P
    from naturaldiffusion_amd import _lib
    from naturaldiffusion_amd.synth import synthetic_inception_head
    _lib.require_gpu()
    out_path = None
    if "--out" in argv:
        i = argv.index("--out"); out_path = argv[i + 1]; del argv[i:i + 2]
    shapes = [tuple(int(v) for v in a.split(":")) for a in argv] or [(50000, 1008, 2048)]
    dev = torch.device("cuda:0")
    results = []
    for n, C, d in shapes:
        x = cluster_feats(n, d, 0.6, 2, dev)
        Wh, bh = synthetic_inception_head(0, C, d)
        head = I.ClassifierHead(Wh, bh, device=dev)
        W, b = Wh.to(dev), bh.to(dev)
        jobs = dict(kernels=lambda: I.inception_score(P.FeatureSet(x), head, group=I.LOCAL)["log_is"][0],
                    torch=lambda: torch_stats(x, W, b)[2])
        values, iters = {}, {}
        for name, fn in jobs.items():                                                   # warm-up at the full shape; the second run's time only sizes the windows
            values[name] = wall(fn)[0]
        for name, fn in jobs.items():
            iters[name] = max(1, round(WINDOW_S / wall(fn)[1]))
        ts = {name: [] for name in jobs}
        for _ in range(REPEATS):                                                        # the jobs alternate
            for name, fn in jobs.items():
                ts[name].append(wall(fn, iters[name])[1])
        med = {name: statistics.median(v) for name, v in ts.items()}
        fs = P.FeatureSet(x)
        med_ms = lambda fn: round(statistics.median(event_ms(fn)[1] for _ in range(REPEATS)), 3)
        parts = dict(planes=med_ms(lambda: P.FeatureSet(x)), row_stats=med_ms(lambda: I.row_stats(fs, None, head)),
                     torch_statements=med_ms(lambda: torch_stats(x, W, b)[0]))
        # the errors on a subset, fp64 on the device
        m = min(SUBSET, n)
        xs = x[:m].contiguous()
        h64, lse64, score64 = torch_stats(xs.double(), W.double(), b.double())
        hk, lsek, _, _ = I.row_stats(P.FeatureSet(xs), None, head)
        ht, lset, score_t = torch_stats(xs, W, b)
        score_k = I.inception_score(xs, head, group=I.LOCAL)["log_is"][0]
        worst = lambda v, ref: float((v.double() - ref).abs().max())
        flop = 2.0 * n * C * d
        res = dict(n=n, classes=C, d=d, seconds={name: spread(v) for name, v in ts.items()}, speedup_of_medians=round(med["torch"] / med["kernels"], 3),
                   repeats=REPEATS, jobs_per_window=iters, parts_ms=parts, kernels_tflops_fp32_equivalent=round(flop / med["kernels"] / 1e12, 1),
                   log_is=dict(kernels=values["kernels"], torch=values["torch"]), subset_rows=m, subset_log_is_fp64=score64,
                   subset_log_is_abs_err=dict(kernels=abs(score_k - score64), torch=abs(score_t - score64)),
                   subset_neg_entropy_abs_err=dict(kernels=worst(hk, h64), torch=worst(ht, h64)),
                   subset_lse_abs_err=dict(kernels=worst(lsek, lse64), torch=worst(lset, lse64)))
        print(json.dumps(res), flush=True)
        results.append(res)
        del x, fs, xs, jobs
        torch.cuda.empty_cache()
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
