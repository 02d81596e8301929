"""Time of the fitter's fp64 Gram kernel (naturaldiffusion_amd/fit.py ``gram``: natinf_fit_gram_f64) beside the plain torch statements on the same device, in
the same process, on the same inputs: the M fp64 vectors of every image stacked ([n, M, epi]: the history rows gathered, noise and target widened) and
``torch.bmm`` of the stack with its transpose.  ``torch_bmm_only`` times the product alone on a stack made beforehand.
usage: bench_fit.py [--out FILE] [n:epi:M ...]        (default: 512:3072:7 512:3072:17)
Times are host clocks around device-synchronised work on device-resident inputs: every side is first run twice; then REPEATS windows of each side alternate
(kernel, torch, product alone, kernel, ...), every window holding as many whole calls as make about WINDOW_S seconds, and the median, the smallest and the
largest time per call are reported.  Error: max over the entries of |G - ref| / sum_e |v_a v_b| of both sides against a longdouble evaluation of SAMPLE
images on the host.  Prints one JSON object per shape (and writes the list to FILE)."""
import json, statistics, sys
from pathlib import Path
import numpy as np
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from bench_prdc import spread, wall

SAMPLE = 4
REPEATS = 7
WINDOW_S = 0.25


def main(argv):
    from naturaldiffusion_amd import fit as F
    from naturaldiffusion_amd import _lib
    _lib.require_gpu()
    out_path = None
    if "--out" in argv:
        i = argv.index("--out"); out_path = argv[i + 1]; del argv[i:i + 2]
    shapes = [tuple(int(v) for v in a.split(":")) for a in argv] or [(512, 3072, 7), (512, 3072, 17)]
    dev = torch.device("cuda:0")
    results = []
    for n, epi, M in shapes:
        n_rows = M - 2
        g = torch.Generator(device=dev).manual_seed(11)
        base = torch.randn(n * epi, generator=g, device=dev, dtype=torch.float64)
        hist = (base[None] + 0.05 * torch.randn(n_rows, n * epi, generator=g, device=dev, dtype=torch.float64)).contiguous()   # nearly parallel rows, as a history's are
        noise = torch.randn(n * epi, generator=g, device=dev)
        target = (base + 0.1 * noise.double()).float()
        rows = list(range(n_rows))

        def kernel():
            return F.gram(hist, rows, noise, target, n, epi)

        def stack():
            return torch.cat([hist.view(n_rows, n, epi).permute(1, 0, 2), noise.double().view(n, 1, epi), target.double().view(n, 1, epi)], 1)

        def statements():
            s = stack()
            return torch.bmm(s, s.transpose(1, 2))

        made = stack()

        def product():
            return torch.bmm(made, made.transpose(1, 2))

        sides = dict(kernel=kernel, torch=statements, torch_bmm_only=product)
        iters = {}
        for name, fn in sides.items():
            wall(fn); wall(fn)
            iters[name] = max(1, round(WINDOW_S / wall(fn, 10)[1]))
        ts = {name: [] for name in sides}
        for _ in range(REPEATS):                                                                # the sides alternate
            for name, fn in sides.items():
                ts[name].append(wall(fn, iters[name])[1])
        v = made[:SAMPLE].cpu().numpy().astype(np.longdouble)
        ref = np.einsum("iae,ibe->iab", v, v)
        mag = np.einsum("iae,ibe->iab", np.abs(v), np.abs(v))
        err = {name: float((np.abs(fn()[:SAMPLE].cpu().numpy().astype(np.longdouble) - ref) / mag).max()) for name, fn in (("kernel", kernel), ("torch", statements))}
        res = dict(n_images=n, elems_per_image=epi, M=M, input_bytes=int(hist.numel() * 8 + 2 * noise.numel() * 4),
                   kernel_s=spread(ts["kernel"], 8), torch_s=spread(ts["torch"], 8), torch_bmm_only_s=spread(ts["torch_bmm_only"], 8),
                   torch_over_kernel_of_medians=round(statistics.median(ts["torch"]) / statistics.median(ts["kernel"]), 3),
                   bmm_only_over_kernel_of_medians=round(statistics.median(ts["torch_bmm_only"]) / statistics.median(ts["kernel"]), 3),
                   kernel_gb_per_s=round((hist.numel() * 8 + 2 * noise.numel() * 4) / statistics.median(ts["kernel"]) / 1e9, 1),
                   repeats=REPEATS, calls_per_window=iters, sample_images=SAMPLE, max_error_over_sum_abs_products=err)
        print(json.dumps(res), flush=True)
        results.append(res)
        del hist, noise, target, made, base
        torch.cuda.empty_cache()
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
