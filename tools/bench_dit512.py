#!/usr/bin/env python3
"""DiT-XL/2 at 512x512 (input size 64, 1,024 tokens) against 256x256 (input 32) in ONE process, device events after warm-up:
  * a forward of 16 at each input size (synthetic weights; the engines' defaults: fused attention, half residual stream);
  * the streaming attention kernel alone at 16 samples x 16 heads x 1,024 tokens x head_dim 72 (natinf_dit_attention_bf16);
  * the per-head GEMM / softmax / GEMM path on the same problem: a depth-1 engine forward with NATINF_DIT_UNFUSED_ATTENTION minus the same
    forward with the fused kernel, plus the fused kernel's own time (the rest of the block is the same launches in both).
Achieved TFLOP/s from shapes: useful FLOPs at hd 72 (4 T^2 hd per head: q k^T and P V) and issued FLOPs at the padded widths (96 for q k^T,
80 for P V).  Writes profiles/dit512/bench_dit512.json (or the path given as the first argument).  --profile-forward: three 512 forwards
of 16 and nothing else (under rocprofv3 --kernel-trace --stats)."""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr          # noqa: E402
from naturaldiffusion_amd.dit import DiTEngine, flatten_state_dict        # noqa: E402
from naturaldiffusion_amd.synth import synthetic_dit_state_dict           # noqa: E402


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def forward_flops(T, B, D=1152, depth=28):
    """2 * MAC: per token 24 D^2 (qkv 6, proj 2, mlp 16) + attention 4 T D per token"""
    return depth * T * (24 * D * D + 4 * T * D) * B


def profile_forward():
    """--profile-forward: only three 512 forwards of 16 (for a kernel-trace run of its own)"""
    sd = synthetic_dit_state_dict(28, 1152, seed=1, input_size=64)
    eng = DiTEngine(flatten_state_dict(sd, 28, 1152), max_batch=16, input_size=64)
    x = torch.randn(16, 4, 64, 64, device="cuda")
    t = torch.full((16,), 500.0, device="cuda")
    y = torch.arange(16, dtype=torch.int32, device="cuda")
    for _ in range(3):
        eng(x, t, y)
    torch.cuda.synchronize()


def main():
    if sys.argv[1:2] == ["--profile-forward"]:
        return profile_forward()
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "dit512" / "bench_dit512.json"
    B, D, H, hd = 16, 1152, 16, 72
    res = {"batch": B, "depth": 28, "hidden": D, "heads": H}
    g = torch.Generator().manual_seed(0)
    for S in (32, 64):
        T = (S // 2) ** 2
        sd = synthetic_dit_state_dict(28, D, seed=1, input_size=S)
        eng = DiTEngine(flatten_state_dict(sd, 28, D), max_batch=B, input_size=S)
        del sd
        x = torch.randn(B, 4, S, S, generator=g).cuda()
        t = torch.full((B,), 500.0, device="cuda")
        y = torch.arange(B, dtype=torch.int32, device="cuda")
        ms = timed(lambda: eng(x, t, y), warm=3, reps=10)
        res[f"forward_input{S}_ms"] = round(ms, 3)
        res[f"forward_input{S}_TFLOPs"] = round(forward_flops(T, B) / ms / 1e9, 1)
        del eng
        torch.cuda.empty_cache()
    res["forward_ratio_64_over_32"] = round(res["forward_input64_ms"] / res["forward_input32_ms"], 3)
    res["flop_ratio_64_over_32"] = round(forward_flops(1024, B) / forward_flops(256, B), 3)

    T = 1024
    qkv = torch.randn(B * T, 3 * D, generator=g).to(torch.bfloat16).cuda()
    o = torch.empty(B * T, D, dtype=torch.bfloat16, device="cuda")
    base = ptr(qkv)
    run = lambda: check(lib.natinf_dit_attention_bf16(base, base + 2 * D, base + 4 * D, 3 * D, ptr(o), D, B, T, H, hd, 0, stream_ptr()), "attn")
    ms_k = timed(run, warm=5, reps=50)
    useful = 4.0 * T * T * hd * B * H
    issued = 2.0 * T * T * (96 + 80) * B * H
    res["attention_kernel_ms"] = round(ms_k, 4)
    res["attention_kernel_TFLOPs_useful"] = round(useful / ms_k / 1e9, 1)
    res["attention_kernel_TFLOPs_issued"] = round(issued / ms_k / 1e9, 1)

    sd = synthetic_dit_state_dict(1, D, seed=2, input_size=64)
    flat = flatten_state_dict(sd, 1, D)
    x = torch.randn(B, 4, 64, 64, generator=g).cuda()
    t = torch.full((B,), 500.0, device="cuda")
    y = torch.arange(B, dtype=torch.int32, device="cuda")
    for name, unf in (("depth1_forward_fused_ms", False), ("depth1_forward_unfused_ms", True)):
        eng = DiTEngine(flat, max_batch=B, depth=1, input_size=64, unfused_attention=unf)
        res[name] = round(timed(lambda: eng(x, t, y), warm=3, reps=10), 3)
        del eng
        torch.cuda.empty_cache()
    res["unfused_attention_path_ms"] = round(res["depth1_forward_unfused_ms"] - res["depth1_forward_fused_ms"] + ms_k, 3)
    res["unfused_over_kernel"] = round(res["unfused_attention_path_ms"] / ms_k, 2)
    res["device"] = torch.cuda.get_device_name(0)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
