"""Throughput of the DiT generation job (ValidateNaturalInference.generate_sharded: counter-based noise, natinf_step_f32prod_noise) on DiT-XL/2 with synthetic weights: images/s for ddim and ddpm at 24 steps, batch sizes 8 / 16 / 32 / 64 (forwards of 16 .. 128 samples), decode off and on, and the engine workspace per batch size; the baseline row is the slab path of natural_inference (torch.randn_like + noise slab, batch 8) timed in the same process.

One JSON object on stdout.  Every row: one untimed warm-up job, then ``--reps`` timed jobs of one batch each, device-synchronised on both
sides; images/s from the median, the spread (min / max seconds) beside it.  GPU box; run from the repository root:

    python tools/dit_job.py [--input-size 64] [--batches 8,16,32,64] [--reps 5]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from naturaldiffusion_amd import ValidateNaturalInference as V                      # noqa: E402
from naturaldiffusion_amd.dit import DiTEngine, flatten_state_dict, XL2           # noqa: E402
from naturaldiffusion_amd.synth import synthetic_dit_state_dict, synthetic_vae_flat  # noqa: E402
from naturaldiffusion_amd.vae import VAEDecoder                                    # noqa: E402


def timed(fn, reps):
    fn()                                                                              # warm-up: allocations, code objects, row tables
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input-size", type=int, default=32, choices=(32, 64))
    ap.add_argument("--batches", default="8,16,32,64")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-decode", action="store_true")
    a = ap.parse_args()
    S = a.input_size
    flat = flatten_state_dict(synthetic_dit_state_dict(input_size=S), XL2["depth"], XL2["hidden"], S)
    vae = None if a.no_decode else VAEDecoder(synthetic_vae_flat(4), max_batch=8, latent_ch=4, latent_res=S)
    rows = []

    def row(path, alg, bs, decode, ws, sec):
        med, lo, hi = sec
        rows.append({"path": path, "alg": alg, "batch_size": bs, "forward_samples": 2 * bs, "decode": decode, "images_per_s": round(bs / med, 2),
                     "median_s": round(med, 4), "min_s": round(lo, 4), "max_s": round(hi, 4), "engine_workspace_bytes": int(ws)})

    # the baseline: natural_inference as it stands (eight demo labels, torch.randn_like copied into the noise slab, natinf_step_f32prod)
    eng = DiTEngine(flat, max_batch=16, input_size=S, **XL2)
    V.denoiser_factory = lambda: eng
    for alg in ("ddim", "ddpm"):
        for decode in ((False,) if vae is None else (False, True)):
            V.decoder_factory = (lambda: (lambda lat, path: V.to_pixels_u8(vae(lat)).cpu())) if decode else None
            row("natural_inference (slab, torch.randn_like)", alg, 8, decode, eng.workspace_bytes, timed(lambda: V.natural_inference(alg, a.steps), a.reps))
    V.denoiser_factory = V.decoder_factory = None
    del eng
    for bs in [int(v) for v in a.batches.split(",")]:
        eng = DiTEngine(flat, max_batch=2 * bs, input_size=S, **XL2)
        for alg in ("ddim", "ddpm"):
            for decode in ((False,) if vae is None else (False, True)):
                job = lambda: V.generate_sharded(bs, None, alg_name=alg, num_step=a.steps, batch_size=bs, seed=0, decode=decode, decode_batch=8,
                                                 model=eng, decoder=vae)
                row("generate_sharded", alg, bs, decode, eng.workspace_bytes, timed(job, a.reps))
        del eng
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "dit_job", "model": "DiT-XL/2 synthetic", "input_size": S, "steps": a.steps, "cfg_scale": 4.0, "reps": a.reps,
                      "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
