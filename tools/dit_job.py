"""Throughput of the DiT generation job (ValidateNaturalInference.generate_sharded: counter-based noise, natinf_step_f32prod_noise) on DiT-XL/2 with synthetic weights: images/s for ddim and ddpm at 24 steps, batch sizes 8 / 16 / 32 / 64 (forwards of 16 .. 128 samples), decode off and on, and the engine workspace per batch size; the baseline row is the slab path of natural_inference (torch.randn_like + noise slab, batch 8) timed in the same process.

One JSON object on stdout.  Every row: one untimed warm-up job, then ``--reps`` timed jobs of one batch each, device-synchronised on both
sides; images/s from the median, the spread (min / max seconds) beside it.  GPU box; run from the repository root:

    python tools/dit_job.py [--input-size 64] [--batches 8,16,32,64] [--reps 5] [--fp8] [--guard | --stream16 auto] [--no-baseline]
                            [--guidance-interval LO HI] [--cfg-scales FILE | 4,1,2.5,...]

``--fp8``: every generate_sharded row is measured twice in the same process -- the bf16 engine, then the engine with fp8 projections (NATINF_DIT_FP8), alternating row by
row -- and carries ``"fp8": false / true``; each (batch size, mode) also gets a ``forwards`` entry: ms per denoiser forward of 2 x batch samples (HIP events over 20
forwards) and the per-shape GEMM table of one forward (natinf_gemm_profile_read: tag, launches, ms, TFLOP/s).

``--guard`` (= ``--stream16 auto``): the cost of the stream guard (NATINF_DIT_STREAM_GUARD).  Every generate_sharded row is measured, alternating in this process, on three
engines per projection mode -- the half stream unguarded (``"stream": "half"``: the default path), the guarded half stream run as ``generate_sharded(stream16="auto")``
(``"half_guarded"``; the synthetic weights stay in range, so no batch reruns -- ``"reruns"`` says so) and the fp32 stream (``"fp32"``: what a rerun costs).

``--guidance-interval LO HI`` / ``--cfg-scales``: the job's guidance arguments (``generate_sharded(guidance_interval=, cfg_scale=<sequence>)``: guide only at the steps whose
timestep lies in LO..HI; one scale per image, 1 = unguided; a list shorter than the batch is cycled over the global index).  Every generate_sharded row is then measured twice,
alternating in this process: ``"guidance": "full"`` -- the default call, [z; z] at every step -- and ``"guidance": "planned"`` -- the job with those arguments; the result's
``guidance`` entry gives, per batch size, the denoiser forward's sample count at each step of the planned job and how many steps guide at all.
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
from naturaldiffusion_amd._lib import lib, check                                    # noqa: E402
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


def forward_profile(eng, n, S):
    """ms per forward of n samples (20 forwards between two events, after 3 untimed) and the GEMM launches of one forward by shape."""
    import ctypes as C
    g = torch.Generator().manual_seed(0)
    z = torch.randn(n, 4, S, S, generator=g).cuda()
    t = torch.linspace(999.0, 3.0, n).cuda()
    y = (torch.arange(n) % 1001).cuda()
    out = torch.empty(n, 8, S, S, device="cuda")
    for _ in range(3):
        eng(z, t, y, out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        eng(z, t, y, out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 20
    check(lib.natinf_gemm_profile(1), "natinf_gemm_profile")
    try:
        eng(z, t, y, out)
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 16)
        rc = lib.natinf_gemm_profile_read(buf, len(buf))
        if rc < 0:
            check(rc, "natinf_gemm_profile_read")
    finally:
        lib.natinf_gemm_profile(0)
    shapes = []
    for line in buf.value.decode().splitlines():
        f = line.split()
        M, N, K0, K1, taps, batch = (int(v) for v in f[:6])
        launches, tot = int(f[7]), float(f[8])
        flop = 2.0 * M * N * (K0 + K1) * batch * launches
        shapes.append({"tag": " ".join(f[:7]), "launches": launches, "ms": round(tot, 4), "tflops": round(flop / (tot * 1e-3) / 1e12, 1) if tot > 0 else None})
    return {"forward_samples": n, "forward_ms": round(ms, 3), "gemms": shapes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input-size", type=int, default=32, choices=(32, 64))
    ap.add_argument("--batches", default="8,16,32,64")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--fp8", action="store_true", help="measure the fp8-projection engine beside the bf16 one, alternating, in this process")
    ap.add_argument("--guard", action="store_true", help="measure the guarded half stream (stream16='auto') and the fp32 stream beside the unguarded half stream, alternating")
    ap.add_argument("--stream16", choices=("auto",), default=None, help="'auto': the same as --guard")
    ap.add_argument("--guidance-interval", type=int, nargs=2, metavar=("LO", "HI"), default=None,
                    help="measure the job with guidance_interval=(LO, HI) beside the full-guidance job, alternating, in this process")
    ap.add_argument("--cfg-scales", default=None, help="per-image CFG scales for the planned job: a file (one number per line or comma separated) or a comma list; cycled over the global index")
    ap.add_argument("--algs", default="ddim,ddpm")
    ap.add_argument("--no-baseline", action="store_true", help="skip the natural_inference (slab) baseline rows")
    a = ap.parse_args()
    a.guard = a.guard or a.stream16 == "auto"
    algs = tuple(a.algs.split(","))
    S = a.input_size
    flat = flatten_state_dict(synthetic_dit_state_dict(input_size=S), XL2["depth"], XL2["hidden"], S)
    vae = None if a.no_decode else VAEDecoder(synthetic_vae_flat(4), max_batch=8, latent_ch=4, latent_res=S)
    rows = []
    planned = a.guidance_interval is not None or a.cfg_scales is not None
    scale_list = None
    if a.cfg_scales is not None:
        text = Path(a.cfg_scales).read_text() if Path(a.cfg_scales).is_file() else a.cfg_scales
        scale_list = [float(v) for v in text.replace(",", " ").split()]
    interval = None if a.guidance_interval is None else tuple(a.guidance_interval)
    guidance = []

    def plan_kw(bs):
        """the planned job's arguments for a batch of bs images"""
        return dict(guidance_interval=interval, cfg_scale=4.0 if scale_list is None else [scale_list[i % len(scale_list)] for i in range(bs)])

    forwards = []

    def row(path, alg, bs, decode, ws, sec, fp8=False, stream=None, reruns=None, mode=None):
        med, lo, hi = sec
        rows.append({"path": path, "alg": alg, "batch_size": bs, "forward_samples": 2 * bs, "decode": decode, "images_per_s": round(bs / med, 2),
                     "median_s": round(med, 4), "min_s": round(lo, 4), "max_s": round(hi, 4), "engine_workspace_bytes": int(ws)})
        if a.fp8:
            rows[-1]["fp8"] = fp8
        if stream is not None:
            rows[-1].update(stream=stream, reruns=reruns)
        if mode is not None:
            rows[-1]["guidance"] = mode                                  # "planned": forward_samples is the largest forward; the per-step sizes are in res["guidance"]

    # the baseline: natural_inference as it stands (eight demo labels, torch.randn_like copied into the noise slab, natinf_step_f32prod)
    eng = DiTEngine(flat, max_batch=16, input_size=S, **XL2)
    V.denoiser_factory = lambda: eng
    for alg in (() if a.no_baseline else algs):
        for decode in ((False,) if vae is None else (False, True)):
            V.decoder_factory = (lambda: (lambda lat, path: V.to_pixels_u8(vae(lat)).cpu())) if decode else None
            row("natural_inference (slab, torch.randn_like)", alg, 8, decode, eng.workspace_bytes, timed(lambda: V.natural_inference(alg, a.steps), a.reps))
    V.denoiser_factory = V.decoder_factory = None
    del eng
    for bs in [int(v) for v in a.batches.split(",")]:
        # (fp8, stream, engine): without --guard one engine per projection mode, the library's default stream
        streams = (("half", dict(stream16=True)), ("half_guarded", dict(stream16=True, guard=True)), ("fp32", dict(stream16=False))) if a.guard else ((None, {}),)
        engines = [(fp8, name, DiTEngine(flat, max_batch=2 * bs, input_size=S, fp8=fp8, **kw, **XL2)) for fp8 in ((False, True) if a.fp8 else (False,)) for name, kw in streams]
        wide = {fp8: eng for fp8, name, eng in engines if name == "fp32"}
        for alg in algs:
            for decode in ((False,) if vae is None else (False, True)):
                for fp8, stream, eng in engines:                              # the modes alternate, row by row
                    rep = {}
                    auto = dict(stream16="auto", fallback=lambda: wide[fp8], report=rep) if stream == "half_guarded" else {}
                    job = lambda **kw: V.generate_sharded(bs, None, alg_name=alg, num_step=a.steps, batch_size=bs, seed=0, decode=decode, decode_batch=8,
                                                          model=eng, decoder=vae, **auto, **kw)
                    if not planned:
                        row("generate_sharded", alg, bs, decode, eng.workspace_bytes, timed(job, a.reps), fp8, stream, len(rep["rerun_batches"]) if auto else None)
                        continue
                    # full guidance and the planned job, alternating job by job: one warm-up each, then reps pairs
                    modes = (("full", {}), ("planned", plan_kw(bs)))
                    secs = {name: [] for name, _ in modes}
                    for name, kw in modes:
                        job(**kw)
                    for _ in range(a.reps):
                        for name, kw in modes:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            job(**kw)
                            torch.cuda.synchronize()
                            secs[name].append(time.perf_counter() - t0)
                    for name, _ in modes:
                        ts = secs[name]
                        row("generate_sharded", alg, bs, decode, eng.workspace_bytes, (statistics.median(ts), min(ts), max(ts)), fp8, stream,
                            len(rep["rerun_batches"]) if auto else None, mode=name)
            if planned:
                C, B, node = V.load_coeff_npz(V.root_path / ("results/%s/%s_%03d.npz" % (alg.replace("_sympy", ""), alg, a.steps)))
                kw = plan_kw(bs)
                guided, slots, _ = V.guidance_plan(node, B.shape[0], V.job_scales(kw["cfg_scale"], bs), interval)
                g = sum(s >= 0 for s in slots)
                guidance.append({"alg": alg, "batch_size": bs, "guided_images": g, "steps_guided": sum(guided), "steps": len(guided),
                                 "timesteps": [int(node[kk, 0]) for kk in range(len(guided))],
                                 "forward_samples_per_step": {"full": [2 * bs] * len(guided), "planned": [bs + g if ok else bs for ok in guided]}})
        if a.fp8 or a.guard:
            for fp8, stream, eng in engines:
                forwards.append(dict(fp8=fp8, batch_size=bs, **({"stream": stream} if stream else {}), **forward_profile(eng, 2 * bs, S)))
        del engines, eng
        torch.cuda.empty_cache()
    res = {"tool": "dit_job", "model": "DiT-XL/2 synthetic", "input_size": S, "steps": a.steps, "cfg_scale": 4.0, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.fp8 or a.guard:
        res["forwards"] = forwards
    if planned:
        res.update(guidance_interval=interval, cfg_scales=scale_list, guidance=guidance)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
