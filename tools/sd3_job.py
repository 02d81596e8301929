"""Throughput of the SD3 generation job (SD3NaturalInference.sd_generate_sharded, BASELINE config 4 / 5 shape) with a guidance interval and with per-image CFG scales against its default form, on the SD3-medium-shaped synthetic engine `bench.py --workload sd3` builds (no diffusers, no weights download): images/s of three forms of one job, and the guided step kernel alone against k_step_f16chain.

One JSON object on stdout.  GPU box; run from the repository root:

    python tools/sd3_job.py [--n 4] [--batches 1] [--reps 3] [--fp8] [--guidance-interval S_LO S_HI] [--cfg-scales 7,1] [--kernel-launches 200] [--blocker-ops 80] [--no-jobs | --no-kernel] [--inpaint]

Jobs.  One job = ``--batches`` batches of ``--n`` images through all 28 steps, no decode.  Three forms, alternating job by job in this process after one untimed
warm-up job each, device-synchronised on both sides; images/s from the median of ``--reps``, the spread (min / max seconds) beside it:
``"default"`` -- none of the new arguments: every step a forward of 2n sequences and natinf_step_f16chain, the path the job always took;
``"interval"`` -- ``guidance_interval=(S_LO, S_HI)`` (default: the middle third of the schedule's steps, sigmas[18] .. sigmas[9]): n sequences at the steps outside;
``"scales"`` -- ``cfg_scale=[...]`` (default 7,1 cycled over the global index: every second image unguided): n + |G| sequences at every step.
``ratio_to_default`` is images/s over the default form's of the same run; ``forward_sequences_per_step`` is what ``sd_guidance_plan`` gives a batch.

Kernel.  natinf_step_f16chain_guided against natinf_step_f16chain at E = 4 x 16 x 128 x 128, k = 27, a dense row (27 history rows and the diagonal), the Euler
flag off.  The guided entry reads its slot table back before it launches, so in a plain back-to-back window the host, not the kernel, sets the pace.  A window is
therefore queued behind a blocker -- ``--blocker-ops`` in-place additions over a 1 GiB tensor, some tens of milliseconds -- and bracketed by two device events:
the host enqueues all ``--kernel-launches`` launches while the GPU is still in the blocker (``host_ahead``: the blocker's event had not completed when the last
launch was enqueued; a window where it had is dropped), so the events time the launches running back to back on the device.  20 untimed launches per form, then
the forms alternate over 5 rounds; microseconds per launch from the median window.  Forms: ``f16chain``; ``guided_identity`` (slots 0..3, one scale: the same
bytes); ``guided_mixed`` (slots -1, 0, -1, 1); ``guided_none`` (every slot -1, v_null NULL).  The blocker leaves the last-level cache cold for a window's first
launch; after it the 68 MB a launch touches stay in the 256 MB cache, for every form alike.

``--inpaint`` measures latent-space inpainting instead, the same way.  Jobs: ``"default"`` against ``"inpaint_fresh"`` and ``"inpaint_same"`` --
``known_latents`` one shared random row, ``mask`` the left half of every channel, ``renoise`` either mode; the forwards are the default form's 2n sequences a step.
Kernel: ``guided_identity`` (natinf_step_f16chain_guided), ``guided_then_blend`` (that launch followed by natinf_known_blend_f16 on its x_next: the two-launch
form the fused step replaces), ``inpaint_fresh`` and ``inpaint_same`` (natinf_step_f16chain_inpaint, the half-image mask), after a check that the fused step's
x_next is the two-launch form's bytes at the timed size.
"""
import argparse
import json
import statistics
import sys
import time
import zlib
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from naturaldiffusion_amd import SD3NaturalInference as S                           # noqa: E402
from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr                   # noqa: E402
from naturaldiffusion_amd.coeff import SparseRows, load_sd3_csv                     # noqa: E402
from naturaldiffusion_amd.mmdit import MMDiTEngine, SD3_MEDIUM                      # noqa: E402
from naturaldiffusion_amd.sampler import KNOWN_COLUMN0                              # noqa: E402
from naturaldiffusion_amd.synth import synthetic_mmdit_flat                         # noqa: E402

NSTEP, TC = 28, 333


def schedule():
    """FlowMatchEulerDiscreteScheduler with shift 3, as bench.py's sd3 workload states it -> (timesteps fp32 [28], sigmas fp32 [29])"""
    u = np.linspace(1.0, 3 * 0.001 / (1 + 2 * 0.001), NSTEP)
    sig = np.append(3 * u / (1 + 2 * u), 0.0).astype(np.float32)
    return torch.from_numpy(sig[:-1] * 1000), torch.from_numpy(sig)


class Pipe:
    """what sd_generate_sharded asks of a pipe: the engine, the schedule, and embeddings that are a function of each prompt string"""

    def __init__(self, n, fp8, dev):
        flat = synthetic_mmdit_flat(grid=64, seed=0, **SD3_MEDIUM)
        self.transformer = MMDiTEngine(flat, max_batch=2 * n, grid=64, ctx_tokens=TC, device=dev, fp8=fp8, **SD3_MEDIUM)
        self.dev = dev

        class Sched:
            def set_timesteps(self, k, device=None):
                assert k == NSTEP
                self.timesteps, self.sigmas = schedule()
        self.scheduler = Sched()

    def _embed(self, text):
        g = torch.Generator().manual_seed(zlib.crc32(text.encode()))
        return torch.randn(TC, 4096, generator=g).half(), torch.randn(2048, generator=g).half()

    def encode_prompt(self, prompt, prompt_2=None, prompt_3=None, negative_prompt=""):
        pos, neg = [self._embed(p) for p in prompt], [self._embed("negative: " + negative_prompt)] * len(prompt)
        st = lambda rows, j: torch.stack([r[j] for r in rows]).to(self.dev)
        return st(pos, 0), st(neg, 0), st(pos, 1), st(neg, 1)


def jobs(a, dev):
    pipe = Pipe(a.n, a.fp8, dev)
    count = a.n * a.batches
    _, sigmas = schedule()
    interval = tuple(a.guidance_interval) if a.guidance_interval else (float(sigmas[18]), float(sigmas[9]))
    scale_list = [float(v) for v in a.cfg_scales.split(",")]
    scales = [scale_list[i % len(scale_list)] for i in range(count)]
    wname = "sd3_step_28_weight_sharp.csv" if a.fp8 else "sd3_step_28_weight.csv"
    forms = (("default", {}), ("interval", dict(guidance_interval=interval)), ("scales", dict(cfg_scale=scales)))
    run = lambda kw: S.sd_generate_sharded(pipe, count, a.n, weight_name=wname, device=dev, **kw)
    secs = {name: [] for name, _ in forms}
    for name, kw in forms:                                                           # warm-up: allocations, code objects, every forward shape of the form
        assert torch.isfinite(run(kw)[0].float()).all(), name
    for _ in range(a.reps):
        for name, kw in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(kw)
            torch.cuda.synchronize()
            secs[name].append(time.perf_counter() - t0)
    rows = []
    base = count / statistics.median(secs["default"])
    for name, kw in forms:
        ts = secs[name]
        guided, slots, _ = S.sd_guidance_plan(sigmas, NSTEP, scales[:a.n] if "cfg_scale" in kw else [7.0] * a.n, kw.get("guidance_interval"))
        g = sum(s >= 0 for s in slots)
        per_step = [2 * a.n] * NSTEP if name == "default" else [a.n + g if on else a.n for on in guided]
        rate = count / statistics.median(ts)
        rows.append({"form": name, "images_per_s": round(rate, 3), "ratio_to_default": round(rate / base, 3), "median_s": round(statistics.median(ts), 4),
                     "min_s": round(min(ts), 4), "max_s": round(max(ts), 4), "steps_guided": NSTEP if name == "default" else sum(guided),
                     "guided_images_per_batch": a.n if name == "default" else g, "sequences_per_job_batch": sum(per_step), "forward_sequences_per_step": per_step})
    return {"images_per_job": count, "batch_size": a.n, "steps": NSTEP, "weights": wname, "guidance_interval": interval, "cfg_scales": scale_list, "rows": rows}


def windows(forms, a, dev):
    """the timed windows of the docstring -> ({form: [microseconds per launch of every window kept]}, windows dropped)"""
    us, dropped = {name: [] for name in forms}, 0
    for fn in forms.values():
        for _ in range(20):
            fn()
    big = torch.zeros(1 << 28, dtype=torch.float32, device=dev)
    for _ in range(5):
        for name, fn in forms.items():
            eb, e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            for _ in range(a.blocker_ops):
                big.add_(1.0)
            eb.record()
            e0.record()
            for _ in range(a.kernel_launches):
                fn()
            e1.record()
            ahead = not eb.query()                                                   # every launch was enqueued while the GPU was still in the blocker
            torch.cuda.synchronize()
            if ahead:
                us[name].append(e0.elapsed_time(e1) * 1e3 / a.kernel_launches)
            else:
                dropped += 1
    assert all(us.values()), "the host never got ahead of the device: raise --blocker-ops"
    return us, dropped


def kernel(a, dev):
    n, se, k = 4, 16 * 128 * 128, 27
    E = n * se
    gen = torch.Generator().manual_seed(0)
    rnd = lambda m: torch.randn(m, generator=gen).half().to(dev)
    x, vt, vn, noise = rnd(E), rnd(E), rnd(E), rnd(E)
    hist = torch.randn(NSTEP, E, generator=gen).half().to(dev)
    mean, xn = torch.empty(E, dtype=torch.float16, device=dev), torch.empty(E, dtype=torch.float16, device=dev)
    rows = SparseRows(load_sd3_csv(S.root_path / "weights" / "sd3_step_28_weight.csv"), lambda j: j + 1, torch.float32, dev, dense=True)
    idx, val, nt = rows.ptrs(k)
    r = rows.rows[k]
    assert nt == k
    sig = (0.05, 0.0, 1.0)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    cfg7 = torch.full((n,), 7.0, device=dev)

    def guided(slots, v_null, g):
        return lambda: check(lib.natinf_step_f16chain_guided(ptr(x), ptr(vt), ptr(v_null), ptr(cfg7), ptr(slots), g, se, ptr(noise), ptr(hist), ptr(mean), ptr(xn),
                                                             idx, val, nt, r.diag, r.total, k, *sig, 0, E, stream_ptr()), "natinf_step_f16chain_guided")
    forms = {"f16chain": lambda: check(lib.natinf_step_f16chain(ptr(x), ptr(vt), ptr(vn), ptr(noise), ptr(hist), ptr(mean), ptr(xn), idx, val, nt, r.diag, r.total,
                                                                k, *sig, 7.0, 0, E, stream_ptr()), "natinf_step_f16chain"),
             "guided_identity": guided(i32([0, 1, 2, 3]), vn, 4), "guided_mixed": guided(i32([-1, 0, -1, 1]), vn, 2), "guided_none": guided(i32([-1] * 4), None, 0)}
    # the same bytes first (the identity rule at the timed size)
    forms["f16chain"]()
    want = (hist[k].clone(), mean.clone(), xn.clone())
    forms["guided_identity"]()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(want, (hist[k], mean, xn))), "the guided kernel's identity rule does not hold at the timed size"
    us, dropped = windows(forms, a, dev)
    # bytes a launch moves: the history rows, x, v_text, noise (and v_null rows) in; hist[k], mean, x_next out
    traffic = lambda rows_null: 2 * (k * E + 3 * E + rows_null * se + 3 * E)
    null_rows = {"f16chain": 4, "guided_identity": 4, "guided_mixed": 2, "guided_none": 0}
    base = statistics.median(us["f16chain"])
    return {"E": E, "k": k, "history_terms": nt, "launches_per_window": a.kernel_launches, "windows_dropped": dropped,
            "rows": [{"form": name, "median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2), "windows": len(t),
                      "ratio_to_f16chain": round(statistics.median(t) / base, 3), "bytes": traffic(null_rows[name]),
                      "tb_per_s": round(traffic(null_rows[name]) / statistics.median(t) / 1e6, 2)} for name, t in us.items()]}


def inpaint_jobs(a, dev):
    pipe = Pipe(a.n, a.fp8, dev)
    count = a.n * a.batches
    wname = "sd3_step_28_weight_sharp.csv" if a.fp8 else "sd3_step_28_weight.csv"
    gen = torch.Generator().manual_seed(1)
    known = torch.randn(1, 16, 128, 128, generator=gen).half()
    mask = torch.zeros(1, 128, 128, dtype=torch.uint8)
    mask[:, :, :64] = 1                                                              # the left half of every channel is known
    forms = (("default", {}), ("inpaint_fresh", dict(known_latents=known, mask=mask, renoise="fresh")),
             ("inpaint_same", dict(known_latents=known, mask=mask, renoise="same")))
    run = lambda kw: S.sd_generate_sharded(pipe, count, a.n, weight_name=wname, device=dev, **kw)
    secs = {name: [] for name, _ in forms}
    for name, kw in forms:                                                           # warm-up, and the result holds the known half
        lat = run(kw)[0]
        assert torch.isfinite(lat.float()).all(), name
        assert not kw or torch.equal(lat[:, :, :, :64], known.to(dev).expand(count, -1, -1, -1)[:, :, :, :64]), name
    for _ in range(a.reps):
        for name, kw in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(kw)
            torch.cuda.synchronize()
            secs[name].append(time.perf_counter() - t0)
    base = count / statistics.median(secs["default"])
    rows = [{"form": name, "images_per_s": round(count / statistics.median(ts), 3), "ratio_to_default": round(count / statistics.median(ts) / base, 3),
             "median_s": round(statistics.median(ts), 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4)} for name, ts in secs.items()]
    return {"images_per_job": count, "batch_size": a.n, "steps": NSTEP, "weights": wname, "mask": "left half, every channel", "rows": rows}


def inpaint_kernel(a, dev):
    n, se, k = 4, 16 * 128 * 128, 27
    E = n * se
    gen = torch.Generator().manual_seed(0)
    rnd = lambda m: torch.randn(m, generator=gen).half().to(dev)
    x, vt, vn, noise, known = rnd(E), rnd(E), rnd(E), rnd(E), rnd(se)
    mask = torch.zeros(16, 128, 128, dtype=torch.uint8)
    mask[:, :, :64] = 1
    mask = mask.reshape(-1).to(dev)
    hist = torch.randn(NSTEP, E, generator=gen).half().to(dev)
    mean, xn = torch.empty(E, dtype=torch.float16, device=dev), torch.empty(E, dtype=torch.float16, device=dev)
    rows = SparseRows(load_sd3_csv(S.root_path / "weights" / "sd3_step_28_weight.csv"), lambda j: j + 1, torch.float32, dev, dense=True)
    idx, val, nt = rows.ptrs(k)
    r = rows.rows[k]
    sig = (0.05, 0.25, 0.75)                                                         # sig, sig_next, 1 - sig_next: exact in fp16
    slots, cfg7, seed = torch.arange(n, dtype=torch.int32, device=dev), torch.full((n,), 7.0, device=dev), 10
    head = (ptr(x), ptr(vt), ptr(vn), ptr(cfg7), ptr(slots), n, se, ptr(noise), ptr(hist), ptr(mean), ptr(xn), idx, val, nt, r.diag, r.total, k, *sig, 0, E)
    col = KNOWN_COLUMN0 + k + 1                                                      # the fresh column of the step's own next level

    def guided():
        check(lib.natinf_step_f16chain_guided(*head, stream_ptr()), "natinf_step_f16chain_guided")

    def blend(column):
        check(lib.natinf_known_blend_f16(ptr(xn), ptr(xn), ptr(noise), ptr(known), ptr(mask), 0, 0, sig[1], sig[2], column, seed, None, 0, 1, se, E, stream_ptr()),
              "natinf_known_blend_f16")

    def fused(column):
        return lambda: check(lib.natinf_step_f16chain_inpaint(*head, ptr(known), ptr(mask), 0, 0, column, seed, None, 0, 1, stream_ptr()), "natinf_step_f16chain_inpaint")

    def two():
        guided()
        blend(col)
    forms = {"guided_identity": guided, "guided_then_blend": two, "inpaint_fresh": fused(col), "inpaint_same": fused(0)}
    for column in (col, 0):                                                          # the same bytes first, at the timed size
        guided()
        blend(column)
        want = xn.clone()
        fused(column)()
        torch.cuda.synchronize()
        assert torch.equal(want, xn), "the fused step is not the guided step followed by the blend at the timed size"
    us, dropped = windows(forms, a, dev)
    base = statistics.median(us["guided_identity"])
    return {"E": E, "k": k, "history_terms": nt, "launches_per_window": a.kernel_launches, "windows_dropped": dropped, "mask": "left half, every channel, one shared row",
            "rows": [{"form": name, "median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2), "windows": len(t),
                      "ratio_to_guided": round(statistics.median(t) / base, 3)} for name, t in us.items()]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4, help="images per batch (the engine takes 2n sequences)")
    ap.add_argument("--batches", type=int, default=1, help="batches per job")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fp8", action="store_true", help="BASELINE config 5: fp8 e4m3 GEMM operands, the sharp weights")
    ap.add_argument("--guidance-interval", type=float, nargs=2, metavar=("S_LO", "S_HI"), default=None)
    ap.add_argument("--cfg-scales", default="7,1", help="comma list, cycled over the global index")
    ap.add_argument("--kernel-launches", type=int, default=200, help="launches per timed window")
    ap.add_argument("--blocker-ops", type=int, default=80, help="1 GiB in-place additions queued ahead of a window")
    ap.add_argument("--no-jobs", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--inpaint", action="store_true", help="measure latent-space inpainting (half-image mask, both renoise modes) instead of the guidance forms")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"tool": "sd3_job", "model": "SD3-medium synthetic (MMDiT 24 blocks, 4,096 + 333 tokens)", "fp8": a.fp8, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    if a.inpaint:
        res["tool"] = "sd3_job --inpaint"
    if not a.no_kernel:
        res["kernel"] = inpaint_kernel(a, dev) if a.inpaint else kernel(a, dev)
    if not a.no_jobs:
        res["jobs"] = inpaint_jobs(a, dev) if a.inpaint else jobs(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
