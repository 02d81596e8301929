"""Encode time of the AutoencoderKL encoder engine (GPU box) and the share of it spent in the k_inc_im2col passes of the three stride-2 convolutions.
usage: bench_vae_encoder.py [latent_res:latent_ch:B ...]       (default: 32:4:16 64:4:16 -- get_feature's two sizes, its batch of 16 -- and 64:16:4)
       bench_vae_encoder.py --stats <*_kernel_stats.csv>       (the share from `rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/bench_vae_encoder.py ...`)
Times come from a host clock around encodes that end in a device synchronise; the share from the kernel records of one more encode under torch.profiler."""
import csv, sys, time
from pathlib import Path
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def share_from_stats(path):
    tot = col = 0.0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            tot += ns
            if "k_inc_im2col" in row["Name"]:
                col += ns
    print(f"{path}: k_inc_im2col {col / 1e6:.3f} ms of {tot / 1e6:.3f} ms kernel time = {100 * col / tot:.1f} %")


def kernel_share(fn):
    """(k_inc_im2col device time, total kernel device time) in microseconds over one call of fn, or None when the profiler recorded no kernel"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    tot = col = 0.0
    for ev in prof.events():
        if str(getattr(ev, "device_type", "")).endswith("CUDA"):
            us = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0)
            tot += us
            if "k_inc_im2col" in ev.name:
                col += us
    return (col, tot) if tot > 0 else None


def main(argv):
    if argv and argv[0] == "--stats":
        return share_from_stats(argv[1])
    from naturaldiffusion_amd.synth import synthetic_vae_encoder_flat
    from naturaldiffusion_amd.vae import VAEEncoder
    cases = [tuple(int(v) for v in a.split(":")) for a in argv] or [(32, 4, 16), (64, 4, 16), (64, 16, 4)]
    for r, ch, B in cases:
        enc = VAEEncoder(synthetic_vae_encoder_flat(ch), max_batch=B, latent_ch=ch, latent_res=r)
        x = torch.rand(B, 3, 8 * r, 8 * r, device="cuda") * 2 - 1
        index = torch.arange(B, device="cuda")
        run = lambda: enc.encode(x, sample=True, scale=0.18215, seed=0, index=index)
        out = run(); torch.cuda.synchronize()
        n = 5
        t0 = time.perf_counter()
        for _ in range(n): out = run()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
        sh = kernel_share(run)
        share = f"k_inc_im2col {sh[0] / 1e3:.3f} ms of {sh[1] / 1e3:.3f} ms kernel time = {100 * sh[0] / sh[1]:.1f} %" if sh else "k_inc_im2col share not measured (no kernel records: use --stats)"
        print(f"images {8 * r}x{8 * r} -> latents {r}x{r}x{ch} B={B}: {ms:.2f} ms per encode, {ms / B:.2f} ms per image, {share}, "
              f"workspace {enc.workspace_bytes / 2 ** 20:.0f} MiB, finite={bool(torch.isfinite(out).all())}", flush=True)
        del enc


if __name__ == "__main__":
    main(sys.argv[1:])
