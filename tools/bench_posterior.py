"""Time and error of the posterior statistics (AnalyzeWeightedSumDegradation.posterior_stats) beside the reference's own statements
(src/AnalyzeWeightedSumDegradation.py:139-146: torch.cdist ... exp ... max) run with torch on the same device, in the same process, on the same inputs.
usage: bench_posterior.py [--out DIR] [n:d ...]        (default: 1300:4096 1300:16384 -- one ImageNet class at 256^2 and at 512^2; DIR default profiles/posterior)
Writes DIR/bench.json and appends to DIR/accuracy.txt.  Times are device events around work on device-resident inputs (after a warm-up of every shape, the
two sides alternating, the median of the repeats); the per-kernel split comes from the kernel records of one more call under torch.profiler; `total` is
posterior_stats itself, host clock, with the upload of the features and the download of the result.  The error is the rms over the rows with an fp64
p_max in (0.05, 0.95) of p - p_fp64, the fp64 evaluation (explicit differences) running on the device as well."""
import json, statistics, sys, time
from pathlib import Path
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

REPEATS = 20


def torch_statements(samples, feats, sigma):
    """the reference's statements, :139-146"""
    exponent = -1 * torch.cdist(samples, feats, p=2) ** 2 / (2 * sigma ** 2)
    max_vals = exponent.max(axis=1, keepdim=True)[0]
    ref_dists = (exponent - max_vals).to(dtype=torch.float64)
    exp_vals = torch.exp(ref_dists, out=ref_dists)
    sum_exp_vals = torch.sum(exp_vals, 1, keepdim=True)
    probs = exp_vals / sum_exp_vals
    return probs.diag(), probs.max(axis=1)[0]


def fp64_statements(samples, feats, sigma):
    d2 = torch.cdist(samples.double(), feats.double(), p=2, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    e = -d2 / (2 * sigma ** 2)
    p = torch.softmax(e, dim=1)
    return p.diag(), p.max(1)[0]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def kernel_times(fn):
    """{kernel name: microseconds} over one call of fn, or {} when the profiler recorded no kernel"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        if str(getattr(ev, "device_type", "")).endswith("CUDA"):
            us = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0)
            name = next((k for k in ("k_post_samples", "k_post_norms", "k_post_dots", "k_post_rows") if k in ev.name), ev.name[:60])
            out[name] = out.get(name, 0.0) + us
    return out


def rms(x):
    return float(torch.sqrt((x.double() ** 2).mean()))


def main(argv):
    from naturaldiffusion_amd import AnalyzeWeightedSumDegradation as A, _lib
    out_dir = ROOT / "profiles" / "posterior"
    if argv and argv[0] == "--out":
        out_dir, argv = Path(argv[1]), argv[2:]
    out_dir.mkdir(parents=True, exist_ok=True)
    cases = [tuple(int(v) for v in a.split(":")) for a in argv] or [(1300, 4096), (1300, 16384)]
    _lib.require_gpu()
    L = _lib.lib
    a, b, sigma = A.level_scalars("vp", 200)
    results, lines = [], []
    for n, d in cases:
        g = torch.Generator().manual_seed(n + d)
        # rows that compete for the posterior (tests/posterior_oracle.py, competing_feats): a common point plus a spread of the noise's size
        feats = (torch.randn(1, d, generator=g, dtype=torch.float64) + (1.5 * b / d ** 0.5) * torch.randn(n, d, generator=g, dtype=torch.float64)).float().bfloat16()
        index = torch.arange(n, dtype=torch.int64)
        smp = A.PosteriorSamples(feats, a, b, seed=1, index=index)
        samples_dev = smp.samples().cuda()
        feats_dev = smp.feats.float()
        idx_dev = index.cuda()
        stats_out = torch.empty((2, n), dtype=torch.float64, device="cuda")

        def run_samples():
            _lib.check(L.natinf_posterior_samples(_lib.ptr(smp.feats), None, a, b, 1, _lib.ptr(idx_dev), 0, 1, n, d, _lib.ptr(smp._ws), _lib.stream_ptr()), "samples")

        def run_stats():
            _lib.check(L.natinf_posterior_stats(_lib.ptr(smp.feats), sigma, n, d, _lib.ptr(smp._ws), _lib.ptr(stats_out[0]), _lib.ptr(stats_out[1]), _lib.stream_ptr()), "stats")

        def run_engine():
            run_samples(); run_stats()

        def run_torch():
            # the reference's side of the same step: the noising statement (:98) on a device-resident noise slab, then :139-146
            return torch_statements(feats_dev * a + noise_dev * b, feats_dev, sigma)

        noise_dev = torch.randn(n, d, device="cuda")
        for _ in range(3):                                    # warm-up: code objects, the library's algorithm choice, the allocator
            run_engine(); run_torch()
        torch.cuda.synchronize()
        t_eng, t_tor, t_smp, t_sta = [], [], [], []
        for _ in range(REPEATS):
            t_eng.append(event_ms(run_engine)); t_tor.append(event_ms(run_torch))
            t_smp.append(event_ms(run_samples)); t_sta.append(event_ms(run_stats))
        t0 = time.perf_counter()
        for _ in range(5):
            A.posterior_stats(feats, a, b, sigma, seed=1, index=index)
        total_ms = (time.perf_counter() - t0) / 5 * 1e3
        kern = kernel_times(run_engine)
        med = statistics.median
        ratio = med(t_tor) / med(t_eng)
        flop = 3 * 2 * n * n * d
        rec = dict(n=n, d=d, engine_ms=med(t_eng), engine_ms_min=min(t_eng), engine_ms_max=max(t_eng), samples_ms=med(t_smp), stats_ms=med(t_sta),
                   torch_ms=med(t_tor), torch_ms_min=min(t_tor), torch_ms_max=max(t_tor), torch_over_engine=ratio,
                   posterior_stats_total_ms=total_ms, kernels_us=kern, repeats=REPEATS,
                   dots_tflops=(flop / (kern["k_post_dots"] * 1e-6) / 1e12 if kern.get("k_post_dots") else None),
                   workspace_mib=int(L.natinf_posterior_workspace_bytes(n, d)) / 2 ** 20)
        # error of both sides on the engine's own samples
        ed, em = fp64_statements(samples_dev, feats_dev, sigma)
        rd, rm = torch_statements(samples_dev, feats_dev, sigma)
        pd, pm = (t.cuda() for t in smp.stats(sigma))
        sel = (em > 0.05) & (em < 0.95)
        rec.update(competing_rows=int(sel.sum()), err_diag_engine=rms((pd - ed)[sel]), err_diag_torch=rms((rd - ed)[sel]),
                   err_max_engine=rms((pm - em)[sel]), err_max_torch=rms((rm - em)[sel]))
        results.append(rec)
        line = (f"bench vp t=200 (n, d) = ({n}, {d}), {rec['competing_rows']} competing rows: rms error p_diag engine {rec['err_diag_engine']:.2e} / torch on the device "
                f"{rec['err_diag_torch']:.2e}; p_max engine {rec['err_max_engine']:.2e} / torch {rec['err_max_torch']:.2e}")
        lines.append(line)
        print(json.dumps(rec), flush=True)
        print(line, flush=True)
        del smp, samples_dev, feats_dev, noise_dev
    (out_dir / "bench.json").write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), level="vp t=200", results=results), indent=1) + "\n")
    with open(out_dir / "accuracy.txt", "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
