"""CPU-side checks: the C-ABI library loads and exports every symbol the headers declare, the engine's
static plan agrees with the oracle's description of the network, and the host logic around the kernels
(sparse coefficient rows, schedules) is right.  No compute call is made (there is no GPU here)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from oracle import ncsnpp_oracle as N
from oracle import ni_oracle as O


def _declared(header_text):
    return set(re.findall(r"\b(natinf_[a-z0-9_]+)\s*\(", header_text))


def test_library_exports_every_declared_symbol(repo_root):
    from naturaldiffusion_amd import _lib
    names = set()
    for h in sorted(p.name for p in (repo_root / "include").glob("natinf*.h")):           # every public header
        names |= _declared((repo_root / "include" / h).read_text())
    names -= {"natinf_stream_t", "natinf_ncsnpp_t", "natinf_dit_t", "natinf_mmdit_t", "natinf_vae_t", "natinf_inception_t"}
    assert len(names) >= 20
    for n in sorted(names):
        assert hasattr(_lib.lib, n), f"libnatinf.so does not export {n}"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert set(_lib.SIGNATURES) <= names
    assert _lib.lib.natinf_abi_version() == 1
    assert _lib.lib.natinf_strerror(-1) == b"invalid argument"


def test_product_does_not_import_the_oracle(repo_root):
    for p in (repo_root / "naturaldiffusion_amd").rglob("*.py"):
        src = p.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), f"{p} imports the oracle"
    for p in (repo_root / "naturaldiffusion_amd" / "csrc").glob("*"):
        if p.is_file():
            assert "oracle" not in p.read_text(errors="ignore").lower() or p.name == "Makefile"


def test_engine_plan_matches_oracle_plan():
    from naturaldiffusion_amd import ncsnpp
    from naturaldiffusion_amd._lib import lib
    tab = ncsnpp.module_table()
    ref = N.plan()
    assert len(tab) == len(ref) == 55
    for row, m in zip(tab, ref):
        idx, kind, cin, cout, up, down, res, poff = row
        assert (idx, kind, cin, cout, bool(up), bool(down), res) == (m.idx, m.kind, m.cin, m.cout, m.up, m.down, m.res)
    shapes = N.param_shapes()
    lay = ncsnpp.param_layout()
    assert [n for n, _ in lay] == list(shapes.keys())
    assert all(tuple(s) == tuple(shapes[n]) for n, s in lay)
    total = sum(int(np.prod(s)) for _, s in lay)
    assert total == lib.natinf_ncsnpp_param_count() == 61804419
    # module parameter offsets are the running sum in that order
    offs = {}
    run = 0
    for n, s in lay:
        i = int(n.split(".")[1])
        offs.setdefault(i, run)
        run += int(np.prod(s))
    assert all(offs[row[0]] == row[7] for row in tab)


def test_workspace_queries():
    from naturaldiffusion_amd._lib import lib
    h = C.c_void_p()
    assert lib.natinf_ncsnpp_create(C.byref(h), 0) == 0
    w1, w512 = lib.natinf_ncsnpp_workspace_bytes(h, 1), lib.natinf_ncsnpp_workspace_bytes(h, 512)
    assert w512 == 512 * w1 and 1e6 < w1 < 2e7
    hk = C.c_void_p()
    assert lib.natinf_ncsnpp_create(C.byref(hk), 1) == 0
    assert lib.natinf_ncsnpp_workspace_bytes(hk, 1) > w1
    assert lib.natinf_ncsnpp_create(C.byref(C.c_void_p()), 4) == -1                  # flags: 1 = keep activations, 2 = the `ddpm` network
    # forward before load -> ESTATE; bad args -> EINVAL (no launch happens)
    assert lib.natinf_ncsnpp_forward(h, 1, 1, 1, 1, 1, 1 << 40, None) == -4
    assert lib.natinf_ncsnpp_forward(h, None, None, None, 1, None, 0, None) == -1
    assert lib.natinf_ncsnpp_destroy(h) == 0 and lib.natinf_ncsnpp_destroy(hk) == 0


def test_flatten_state_dict_and_ema_order():
    from naturaldiffusion_amd import ncsnpp
    shapes = N.param_shapes()
    sd = {"module." + k: torch.full(s, float(i)) for i, (k, s) in enumerate(shapes.items())}
    flat = ncsnpp.flatten_state_dict(sd)
    ema = ncsnpp.flatten_ema([torch.full(s, float(i)) for i, s in enumerate(shapes.values())])
    assert flat.numel() == 61804419 and torch.equal(flat, ema)
    with pytest.raises(ValueError):
        ncsnpp.flatten_state_dict({**sd, "module.all_modules.2.weight": torch.zeros(128, 3, 1, 1)})
    with pytest.raises(KeyError):
        ncsnpp.flatten_state_dict({k: v for k, v in sd.items() if not k.endswith("all_modules.54.bias")})


def test_sparse_rows(repo_root):
    from naturaldiffusion_amd.coeff import SparseRows, load_coeff_npz, load_sd3_csv
    C_, B_, node = load_coeff_npz(repo_root / "weights/step_15_weight_173.npz")
    for dense in (False, True):
        rows = SparseRows(C_, lambda k: k + 1, torch.float64, None, dense=dense)
        for k, r in enumerate(rows.rows):
            idx = rows.idx_host[r.start:r.start + r.n]
            val = rows.val_host[r.start:r.start + r.n]
            assert np.all(np.diff(idx) > 0) and (r.n == 0 or idx.max() < k)
            assert r.diag == C_[k, k]
            rebuilt = np.zeros(k + 1)
            rebuilt[idx] = val
            rebuilt[k] = r.diag
            assert np.array_equal(rebuilt, C_[k, :k + 1])
            assert r.n == (k if dense else np.count_nonzero(C_[k, :k]))
    W = load_sd3_csv(repo_root / "weights/sd3_step_28_weight.csv")
    rows = SparseRows(W, lambda k: k + 1, torch.float32, None)
    assert rows.val_host.dtype == np.float32
    tot = 0
    for j in range(28):
        tot = tot + W[27][j]
    assert rows.rows[27].total == float(tot)
    with pytest.raises(ValueError):
        load_coeff_npz(repo_root / "tests/golden/cifar_form.npz")


def test_host_schedule_matches_oracle(repo_root):
    from naturaldiffusion_amd.sampler import vp_std_f32
    from naturaldiffusion_amd.coeff import load_coeff_npz
    _, _, node = load_coeff_npz(repo_root / "weights/step_10_weight_42.npz")
    for t in node[:-1, 0]:
        assert vp_std_f32(t) == float(O.vp_std_f32(t))


def test_gpu_required_is_loud():
    from naturaldiffusion_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.require_gpu()
    from naturaldiffusion_amd.sampler import CifarNI
    with pytest.raises(RuntimeError):
        CifarNI(np.eye(2), np.ones((2, 2)), np.ones((3, 3)), 8)


def test_synthetic_weights_match_the_oracle_recipe():
    """bench.py feeds the GPU engine from naturaldiffusion_amd.synth and its CPU baseline from the oracle:
    the two generators must produce the same tensors."""
    from naturaldiffusion_amd.synth import synthetic_state_dict
    a, b = synthetic_state_dict(0), N.make_params(0)
    assert list(a) == list(b)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_synthetic_dit_weights_match_the_oracle_recipe():
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.synth import synthetic_dit_state_dict
    from naturaldiffusion_amd.dit import param_layout
    a, b = synthetic_dit_state_dict(2, 128, seed=7), D.make_params(2, 128, seed=7)
    assert list(a) == list(b) == [n for n, _ in param_layout(2, 128)]
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_synthetic_mmdit_weights_match_the_oracle_recipe():
    from oracle import mmdit_oracle as M
    from naturaldiffusion_amd.synth import synthetic_mmdit_flat
    from naturaldiffusion_amd.mmdit import flatten_state_dict
    cfg = dict(layers=2, heads=2, joint_dim=64, pooled_dim=32)
    a = synthetic_mmdit_flat(grid=8, seed=5, pos_max=24, pos_base=8, **cfg)
    b = flatten_state_dict(M.make_params(seed=5, pos_max=24, pos_base=8, **cfg), 8, **cfg)
    assert torch.equal(a, b)


def test_vae_loader_accepts_pre_rename_attention_keys():
    """The 2022 sd-vae-ft-* weight files keep the mid-block attention under query / key / value / proj_attn (some as 1x1
    conv weights); AutoencoderKL.from_pretrained renames them on load (reference ValidateNaturalInference.py:212-214 goes
    through it), so the raw-file loader must as well."""
    import torch
    from naturaldiffusion_amd.vae import flatten_state_dict, param_layout
    g = torch.Generator().manual_seed(2)
    new = {"decoder." + n: torch.randn(s, generator=g) for n, s in param_layout(4)}
    new["post_quant_conv.weight"] = torch.randn(4, 4, 1, 1, generator=g)
    new["post_quant_conv.bias"] = torch.randn(4, generator=g)
    old = {}
    for k, v in new.items():
        for a, b in (("to_q", "query"), ("to_k", "key"), ("to_v", "value"), ("to_out.0", "proj_attn")):
            if f".attentions.0.{a}." in k:
                k = k.replace(f".attentions.0.{a}.", f".attentions.0.{b}.")
                if k.endswith("weight") and b in ("query", "proj_attn"):
                    v = v[:, :, None, None]                 # conv-style storage of the same matrix
        old[k] = v
    assert any(".query." in k for k in old) and not any(".to_q." in k for k in old)
    assert torch.equal(flatten_state_dict(old, 4, prefix="decoder."), flatten_state_dict(new, 4, prefix="decoder."))


def test_attention_abi_rejects_padding_beyond_the_masked_tile():
    """natinf_attention_hd64_bf16 masks only the last 128-key tile: Tp - T >= 128 must be an argument error, not a wrong
    softmax (include/natinf_mmdit.h)."""
    from naturaldiffusion_amd._lib import lib
    dummy = 4096
    assert lib.natinf_attention_hd64_bf16(dummy, dummy, 64, 256 * 64, dummy, dummy, 64, 256 * 64, 1, 1, 256, 128, 0.125, None) == -1
    assert lib.natinf_attention_hd64_bf16(dummy, dummy, 64, 256 * 64, dummy, dummy, 64, 256 * 64, 1, 1, 256, 300, 0.125, None) == -1


def test_attention_fp8out_hook_rejects_bad_arguments():
    """natinf_debug_attention_hd64_fp8out (include/natinf_mmdit.h): the refusals of natinf_attention_hd64_bf16, plus NULL o8 / omx and an odd head count (a scale
    plane pairs heads) -- NATINF_EINVAL before anything is configured or launched (there is no GPU here)."""
    from naturaldiffusion_amd._lib import lib
    d = 4096                                                # a non-NULL dummy: never dereferenced by the argument check
    names = ("q", "k", "ld_qk", "qk_bs", "vT", "o8", "omx", "B", "H", "Tp", "T", "scale", "stream")
    call = lambda **kw: lib.natinf_debug_attention_hd64_fp8out(*[{**dict(q=d, k=d, ld_qk=128, qk_bs=256 * 128, vT=d, o8=d, omx=d, B=1, H=2, Tp=256, T=200, scale=0.125,
                                                                         stream=None), **kw}[n] for n in names])
    assert call(T=128) == -1 and call(T=300) == -1          # padding beyond the masked tile; more keys than rows
    for name in ("q", "k", "vT", "o8", "omx"):
        assert call(**{name: None}) == -1
    for H in (1, 3, 0, -2):
        assert call(H=H) == -1
    assert call(B=0) == -1 and call(Tp=200) == -1 and call(Tp=0) == -1 and call(T=0) == -1 and call(ld_qk=132) == -1


def test_attention_block_hook_rejects_bad_arguments():
    """natinf_debug_attn_block (include/natinf_ncsnpp.h): every argument error is NATINF_EINVAL before anything is configured or launched (there is no GPU here)."""
    from naturaldiffusion_amd._lib import lib
    d = 4096                                                # a non-NULL dummy: never dereferenced by the argument check
    call = lambda **kw: lib.natinf_debug_attn_block(*[{**dict(plan=2, B=1, x=d, x_ld=256, scale=d, shift=d, w=d, bias=d, packed=d, scratch=d, out=d, o_ld=256,
                                                                out_scale=1.0, gn_part=None, stream=None), **kw}[k]
                                                      for k in ("plan", "B", "x", "x_ld", "scale", "shift", "w", "bias", "packed", "scratch", "out", "o_ld", "out_scale", "gn_part", "stream")])
    for plan in (-1, 3):
        assert call(plan=plan) == -1
    for B in (0, -2):
        assert call(B=B) == -1
    for ld in (0, 248, 255, 260, 388):                      # below 256, or not a multiple of 8
        assert call(x_ld=ld) == -1 and call(o_ld=ld) == -1
    for name in ("x", "scale", "shift", "w", "bias", "packed", "out"):
        for plan in (0, 1, 2):
            assert call(plan=plan, **{name: None}) == -1, name
    assert call(plan=0, scratch=None) == -1 and call(plan=1, scratch=None) == -1      # (plan 2 needs no scratch)


def test_ln_modulate_hook_rejects_bad_arguments():
    """natinf_debug_ln_modulate (include/natinf_dit.h): every argument error is NATINF_EINVAL before anything is launched (there is no GPU here)."""
    from naturaldiffusion_amd._lib import lib
    d = 4096                                                # a non-NULL, 16-byte aligned dummy: never dereferenced by the argument check
    form = C.c_int(-7)
    names = ("x", "x_f16", "shift", "scale", "mod_ld", "h_bf16", "h_fp8", "row_scale", "D", "rows", "rows_per_sample", "form_out", "stream")
    base = dict(x=d, x_f16=0, shift=d, scale=d, mod_ld=6 * 256, h_bf16=None, h_fp8=None, row_scale=None, D=256, rows=15, rows_per_sample=5, form_out=C.byref(form),
                stream=None)
    for out in (dict(h_bf16=d), dict(h_fp8=d, row_scale=d)):
        call = lambda **kw: lib.natinf_debug_ln_modulate(*[{**base, **out, **kw}[n] for n in names])
        for name in ("x", "shift", "scale", "form_out", *out):
            assert call(**{name: None}) == -1, name
        for D in (0, -64, 1536 + 128, 1600, 96, 257):
            assert call(D=D, mod_ld=6 * 1600) == -1, D
        for x_f16 in (0, 1):
            assert call(rows=0, x_f16=x_f16) == -1 and call(rows=-3) == -1 and call(rows_per_sample=0) == -1 and call(rows_per_sample=-5) == -1
        assert call(mod_ld=255) == -1 and call(mod_ld=0) == -1
        assert call(x=d + 4) == -1 and call(x=d + 8) == -1 and call(**{next(iter(out)): d + 8}) == -1      # x, the output: 16-byte aligned
    call = lambda **kw: lib.natinf_debug_ln_modulate(*[{**base, **kw}[n] for n in names])
    assert call() == -1                                                                                     # neither output
    assert call(h_bf16=d, h_fp8=d, row_scale=d) == -1 and call(h_bf16=d, h_fp8=d) == -1 and call(h_bf16=d, row_scale=d) == -1      # both
    assert call(h_fp8=d) == -1 and call(row_scale=d) == -1                                                 # half of the fp8 pair
    assert call(h_fp8=d, row_scale=d, D=64, mod_ld=384) == -1 and call(h_fp8=d, row_scale=d, D=192, mod_ld=6 * 192) == -1      # fp8: whole 128-column groups
    assert form.value == -7                                                                                # a refusal leaves *form_out alone


def test_softmax_rows_hook_rejects_bad_arguments():
    """natinf_debug_softmax_rows (include/natinf_dit.h): NATINF_EINVAL outside each kernel's stated contract, before anything is launched."""
    from naturaldiffusion_amd._lib import lib
    d = 4096
    call = lambda **kw: lib.natinf_debug_softmax_rows(*[{**dict(kind=0, S=d, P=d, T=64, rows=7, stream=None), **kw}[n] for n in ("kind", "S", "P", "T", "rows", "stream")])
    for kind in (-1, 3):
        assert call(kind=kind) == -1
    for kind in (0, 1, 2):
        assert call(kind=kind, S=None) == -1 and call(kind=kind, P=None) == -1 and call(kind=kind, rows=0) == -1 and call(kind=kind, rows=-1) == -1
        assert call(kind=kind, T=0) == -1 and call(kind=kind, T=-64) == -1
    for T in (260, 320, 1024, 18, 30, 255, 8 + 1):          # kind 0: T <= 256 and (T % 4 == 0 or T == 16)
        assert call(kind=0, T=T) == -1, T
    for T in (16, 100, 32, 1024 + 64, 4096):                # kind 1: T % 64 == 0 and T <= 1024
        assert call(kind=1, T=T) == -1, T
    for T in (16, 100, 1088 + 32, 4097):                    # kind 2: T % 64 == 0
        assert call(kind=2, T=T) == -1, T


def test_inception_kernel_hooks_reject_bad_arguments():
    """natinf_debug_inc_stem / _pool / _global_avg / _pack / _im2col (include/natinf_inception.h): NATINF_EINVAL outside each stated contract, before anything is
    launched (there is no GPU here)."""
    from naturaldiffusion_amd._lib import lib
    d = 4096                                                # a non-NULL, 16-byte aligned dummy: never dereferenced by the argument check

    def caller(fn, names, base):
        return lambda **kw: fn(*[{**base, **kw}[n] for n in names])

    call = caller(lib.natinf_debug_inc_stem, ("images", "input_kind", "B", "H", "W", "f16", "row_width", "out", "stream"),
                  dict(images=d, input_kind=0, B=2, H=32, W=32, f16=1, row_width=32, out=d, stream=None))
    assert call(images=None) == -1 and call(out=None) == -1 and call(out=d + 4) == -1 and call(input_kind=1, images=d + 2) == -1
    for bad in (dict(input_kind=-1), dict(input_kind=2), dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-5), dict(H=4097), dict(W=4097), dict(f16=2), dict(f16=-1),
                dict(row_width=0), dict(row_width=16), dict(row_width=48), dict(row_width=128), dict(B=(1 << 31) // (149 * 149) + 1)):
        assert call(**bad) == -1, bad

    call = caller(lib.natinf_debug_inc_pool, ("f16", "mode", "stride", "pad", "B", "H", "W", "C", "x", "x_ld", "out", "out_ld", "stream"),
                  dict(f16=0, mode=1, stride=1, pad=1, B=2, H=8, W=8, C=72, x=d, x_ld=80, out=d, out_ld=80, stream=None))
    assert call(x=None) == -1 and call(out=None) == -1 and call(x=d + 8) == -1 and call(out=d + 8) == -1
    for bad in (dict(f16=2), dict(mode=2), dict(mode=-1), dict(stride=0), dict(stride=3), dict(pad=-1), dict(pad=2), dict(B=0), dict(H=0), dict(W=0), dict(H=65537),
                dict(C=0), dict(C=4), dict(C=76), dict(x_ld=64), dict(x_ld=76), dict(out_ld=64), dict(out_ld=84),
                dict(pad=0, H=2), dict(pad=0, W=2), dict(pad=0, H=1, stride=2), dict(pad=0, W=1, stride=2),          # Ho / Wo < 1 (1 - 3 rounds toward zero in C)
                dict(B=1 << 20, H=65536, C=8 * 64, x_ld=512, out_ld=512)):                                           # 2^42 threads
        assert call(**bad) == -1, bad

    call = caller(lib.natinf_debug_inc_global_avg, ("f16", "B", "HW", "C", "x", "out", "stream"), dict(f16=0, B=2, HW=64, C=2048, x=d, out=d, stream=None))
    for bad in (dict(x=None), dict(out=None), dict(x=d + 1), dict(out=d + 2), dict(f16=2), dict(B=0), dict(HW=0), dict(C=0), dict(B=-1), dict(HW=-64), dict(C=-8),
                dict(B=1 << 16, C=1 << 15)):
        assert call(**bad) == -1, bad

    names = ("f16", "w", "gamma", "beta", "mean", "var", "N", "Np", "C", "Cp", "kh", "kw", "Kp", "wp", "bias", "deq", "stream")
    base = dict(f16=0, w=d, gamma=d, beta=d, mean=d, var=d, N=48, Np=64, C=40, Cp=64, kh=1, kw=7, Kp=448, wp=d, bias=d, deq=None, stream=None)
    for f16 in (0, 1):
        call = caller(lib.natinf_debug_inc_pack, names, {**base, "f16": f16, "deq": d if f16 else None})
        for name in ("w", "gamma", "beta", "mean", "var", "wp", "bias"):
            assert call(**{name: None}) == -1, name
        for bad in (dict(f16=2), dict(N=0), dict(Np=47), dict(C=0), dict(Cp=39), dict(kh=0), dict(kw=0), dict(Kp=0), dict(Kp=447), dict(Kp=416), dict(Kp=440),
                    dict(w=d + 2), dict(bias=d + 2), dict(wp=d + 1), dict(Np=1 << 20, Kp=1 << 11)):
            assert call(**bad) == -1, bad
    assert call(deq=None) == -1 and call(deq=d + 2) == -1                                                 # the half pack needs its scales

    call = caller(lib.natinf_debug_inc_im2col, ("B", "H", "W", "ld", "C", "kh", "kw", "stride", "ph", "pw", "Kp", "x", "out", "stream"),
                  dict(B=2, H=17, W=17, ld=128, C=128, kh=3, kw=3, stride=2, ph=0, pw=0, Kp=1152, x=d, out=d, stream=None))
    for bad in (dict(x=None), dict(out=None), dict(x=d + 8), dict(out=d + 8), dict(B=0), dict(H=0), dict(W=0), dict(H=65537), dict(kh=0), dict(kw=0), dict(stride=0),
                dict(ph=-1), dict(pw=-1), dict(ph=4097), dict(C=0), dict(C=4), dict(C=124), dict(ld=120), dict(ld=132), dict(Kp=1144), dict(Kp=1156), dict(Kp=0),
                dict(H=2), dict(W=2), dict(H=1, stride=4), dict(B=1 << 14, H=1025, W=1025, stride=1)):
        assert call(**bad) == -1, bad


def test_gn_kernel_hooks_reject_bad_arguments():
    """natinf_debug_gn_stats / _gn_finalize / _gn_fold / _gn_apply / _head_conv / _time_embed / _stem_im2col / _pack_conv / _pack_transpose / _nhwc_to_nchw
    (include/natinf_ncsnpp.h): NATINF_EINVAL outside the preconditions each kernel leaves to its caller, before anything is launched (there is no GPU here)."""
    from naturaldiffusion_amd._lib import lib
    d = 4096

    def caller(fn, names, base):
        return lambda **kw: fn(*[{**base, **kw}[n] for n in names])

    call = caller(lib.natinf_debug_gn_stats, ("x", "ld", "C", "HW", "B", "gamma", "beta", "scale", "shift", "eps", "out_mul", "stream"),
                  dict(x=d, ld=128, C=128, HW=64, B=2, gamma=d, beta=d, scale=d, shift=d, eps=1e-6, out_mul=1.0, stream=None))
    for name in ("x", "gamma", "beta", "scale", "shift"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(C=0), dict(C=16), dict(C=120), dict(C=136, ld=136), dict(C=544, ld=544), dict(C=1024, ld=1024), dict(ld=120), dict(ld=132), dict(HW=0), dict(B=0),
                dict(x=d + 8)):
        assert call(**bad) == -1, bad

    names = ("P0", "tps0", "quads0", "P1", "tps1", "quads1", "C", "HW", "B", "gamma", "beta", "scale", "shift", "eps", "out_mul", "stream")
    base = dict(P0=d, tps0=4, quads0=64, P1=None, tps1=0, quads1=0, C=256, HW=256, B=2, gamma=d, beta=d, scale=d, shift=d, eps=1e-6, out_mul=1.0, stream=None)
    call = caller(lib.natinf_debug_gn_finalize, names, base)
    for name in ("P0", "gamma", "beta", "scale", "shift"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(C=64, quads0=16), dict(C=96, quads0=24), dict(C=192, quads0=48), dict(C=320, quads0=80),      # C % 128: qpg would be 0 or drop a quad
                dict(C=640, quads0=160), dict(C=1024, quads0=256), dict(quads0=32), dict(quads0=128), dict(tps0=0), dict(HW=0), dict(B=0),
                dict(tps1=2), dict(quads1=32, C=384), dict(P1=d, tps1=2, quads1=0), dict(P1=d, tps1=0, quads1=32, C=384), dict(P1=d, tps1=2, quads1=32),
                dict(P1=d, tps1=2, quads1=96, C=640), dict(P0=d + 4), dict(P1=d + 4, tps1=2, quads1=32, C=384)):
        assert call(**bad) == -1, bad

    call = caller(lib.natinf_debug_gn_fold, ("P", "tps", "quads", "fold", "B", "out", "stream"), dict(P=d, tps=320, quads=64, fold=5, B=2, out=d, stream=None))
    for bad in (dict(P=None), dict(out=None), dict(quads=96), dict(quads=48), dict(quads=0), dict(quads=512), dict(fold=0), dict(fold=3), dict(tps=4), dict(B=0),
                dict(B=65536), dict(P=d + 4), dict(out=d + 4)):      # quads = 96 (C = 384): a third, partial lane would add tiles twice
        assert call(**bad) == -1, bad

    names = ("x", "ld", "C", "logW", "logHW", "B", "scale", "shift", "y", "xr", "act", "mode", "pad", "stream")
    call = caller(lib.natinf_debug_gn_apply, names, dict(x=d, ld=128, C=128, logW=3, logHW=6, B=2, scale=d, shift=d, y=d, xr=None, act=1, mode=0, pad=1, stream=None))
    for name in ("x", "scale", "shift", "y"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(C=0), dict(C=4), dict(C=100), dict(C=2056, ld=2056), dict(ld=120), dict(ld=132), dict(B=0), dict(B=65536), dict(logW=-1), dict(logHW=2),
                dict(logHW=25), dict(mode=3), dict(mode=-1), dict(pad=2), dict(pad=-1), dict(act=2), dict(act=-1), dict(mode=2, logW=0, logHW=0),
                dict(scale=d + 4), dict(shift=d + 8), dict(x=d + 8), dict(y=d + 8), dict(xr=d + 8)):
        assert call(**bad) == -1, bad

    call = caller(lib.natinf_debug_head_conv, ("x", "ld", "B", "scale", "shift", "w16", "bias", "out", "stream"),
                  dict(x=d, ld=128, B=2, scale=d, shift=d, w16=d, bias=d, out=d, stream=None))
    for name in ("x", "scale", "shift", "w16", "bias", "out"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(ld=120), dict(ld=132), dict(B=0), dict(x=d + 8), dict(w16=d + 8), dict(out=d + 4)):
        assert call(**bad) == -1, bad

    assert lib.natinf_debug_time_embed(None, d, 2, None) == -1 and lib.natinf_debug_time_embed(d, None, 2, None) == -1
    assert lib.natinf_debug_time_embed(d, d, 0, None) == -1 and lib.natinf_debug_time_embed(d, d, 1 << 21, None) == -1
    assert lib.natinf_debug_stem_im2col(None, d, 2, None) == -1 and lib.natinf_debug_stem_im2col(d, None, 2, None) == -1
    assert lib.natinf_debug_stem_im2col(d, d, 0, None) == -1 and lib.natinf_debug_stem_im2col(d, d + 8, 2, None) == -1

    names = ("src", "dst", "N", "Cin", "taps", "dst_ld", "koff", "tap_stride_c", "chunked", "wmul", "stream")
    call = caller(lib.natinf_debug_pack_conv, names, dict(src=d, dst=d, N=3, Cin=128, taps=9, dst_ld=1152, koff=0, tap_stride_c=128, chunked=1, wmul=1.0, stream=None))
    for bad in (dict(src=None), dict(dst=None), dict(N=0), dict(Cin=0), dict(taps=0), dict(koff=-1), dict(chunked=2), dict(dst_ld=1151), dict(koff=1),
                dict(Cin=129), dict(chunked=0, tap_stride_c=127), dict(chunked=0, dst_ld=1151), dict(chunked=0, Cin=3, tap_stride_c=3, dst_ld=26)):
        assert call(**bad) == -1, bad
    call = caller(lib.natinf_debug_pack_transpose, ("src", "dst", "K", "N", "dst_ld", "stream"), dict(src=d, dst=d, K=40, N=24, dst_ld=48, stream=None))
    for bad in (dict(src=None), dict(dst=None), dict(K=0), dict(N=0), dict(dst_ld=39)):
        assert call(**bad) == -1, bad
    call = caller(lib.natinf_debug_nhwc_to_nchw, ("x", "ld", "C", "HW", "B", "out", "stream"), dict(x=d, ld=48, C=40, HW=12, B=2, out=d, stream=None))
    for bad in (dict(x=None), dict(out=None), dict(C=0), dict(HW=0), dict(B=0), dict(ld=39)):
        assert call(**bad) == -1, bad


def test_glue_kernel_hooks_reject_bad_arguments():
    """natinf_debug_patch_embed / _dit_time_freq / _dit_cond / _silu_bf16 / _f32_to_bf16 / _unpatchify (include/natinf_dit.h) and natinf_debug_vae_latents / _vae_images /
    _vae_quant (include/natinf_vae.h): NATINF_EINVAL outside each stated contract, before anything is launched (there is no GPU here)."""
    from naturaldiffusion_amd._lib import lib
    d = 4096                                                # a non-NULL, 16-byte aligned dummy: never dereferenced by the argument check

    def caller(fn, names, base):
        return lambda **kw: fn(*[{**base, **kw}[n] for n in names])

    names = ("z", "w", "wt", "bias", "pos", "x", "x_f16", "guard", "C", "g", "D", "B", "stream")
    for x_f16 in (0, 1):
        for guard in (None, d):
            call = caller(lib.natinf_debug_patch_embed, names, dict(z=d, w=d, wt=d, bias=d, pos=d, x=d, x_f16=x_f16, guard=guard, C=4, g=3, D=320, B=3, stream=None))
            for name in ("z", "w", "wt", "bias", "pos", "x"):
                assert call(**{name: None}) == -1, name
            for bad in (dict(C=0), dict(C=-4), dict(C=17), dict(C=64), dict(g=0), dict(g=-1), dict(g=257), dict(D=0), dict(D=-64), dict(D=32), dict(D=96), dict(D=330),
                        dict(D=1600), dict(D=2048), dict(B=0), dict(B=-2), dict(g=256, B=17), dict(B=1 << 30), dict(x=d + 1), dict(guard=d + 2)):
                assert call(**bad) == -1, bad
            if not x_f16:
                assert call(x=d + 2) == -1                                        # an fp32 stream is 4-byte aligned (a half stream 2-byte: d + 1 above)

    call = caller(lib.natinf_debug_dit_time_freq, ("t", "emb", "B", "stream"), dict(t=d, emb=d, B=3, stream=None))
    for bad in (dict(t=None), dict(emb=None), dict(B=0), dict(B=-1), dict(B=(1 << 22) + 1)):
        assert call(**bad) == -1, bad
    call = caller(lib.natinf_debug_dit_cond, ("c0", "table", "y", "cs", "D", "B", "stream"), dict(c0=d, table=d, y=d, cs=d, D=1152, B=3, stream=None))
    for bad in (dict(c0=None), dict(table=None), dict(y=None), dict(cs=None), dict(D=0), dict(D=-64), dict(B=0), dict(B=-3), dict(D=1 << 16, B=1 << 15)):
        assert call(**bad) == -1, bad
    for fn in (lib.natinf_debug_silu_bf16, lib.natinf_debug_f32_to_bf16):
        assert fn(None, d, 5, None) == -1 and fn(d, None, 5, None) == -1 and fn(d, d, 0, None) == -1 and fn(d, d, -7, None) == -1 and fn(d, d, 1 << 31, None) == -1
    call = caller(lib.natinf_debug_unpatchify, ("tok", "out", "OC", "g", "n_images", "stream"), dict(tok=d, out=d, OC=8, g=16, n_images=2, stream=None))
    for bad in (dict(tok=None), dict(out=None), dict(OC=0), dict(OC=-8), dict(OC=4097), dict(g=0), dict(g=-1), dict(g=4097), dict(n_images=0), dict(n_images=-2),
                dict(OC=4096, g=4096), dict(n_images=1 << 22, g=16)):
        assert call(**bad) == -1, bad

    call = caller(lib.natinf_debug_vae_latents, ("z", "W", "bias", "y", "C", "r", "B", "stream"), dict(z=d, W=d, bias=d, y=d, C=4, r=8, B=2, stream=None))
    for bad in (dict(z=None), dict(W=None), dict(bias=None), dict(y=None), dict(y=d + 1), dict(C=0), dict(C=-4), dict(C=65), dict(r=0), dict(r=-8), dict(r=4097), dict(B=0),
                dict(B=-1), dict(r=4096, B=2)):
        assert call(**bad) == -1, bad
    call = caller(lib.natinf_debug_vae_images, ("img", "y", "R", "B", "stream"), dict(img=d, y=d, R=17, B=2, stream=None))
    for bad in (dict(img=None), dict(y=None), dict(y=d + 8), dict(y=d + 2), dict(R=0), dict(R=-1), dict(R=16385), dict(B=0), dict(B=-2), dict(R=8192, B=1)):
        assert call(**bad) == -1, bad
    call = caller(lib.natinf_debug_vae_quant, ("m", "W", "bias", "out", "N", "hw", "B", "stream"), dict(m=d, W=d, bias=d, out=d, N=8, hw=63, B=2, stream=None))
    for bad in (dict(m=None), dict(W=None), dict(bias=None), dict(out=None), dict(N=0), dict(N=-2), dict(N=65), dict(hw=0), dict(hw=-64), dict(B=0), dict(B=-1),
                dict(N=64, hw=1 << 24, B=2)):
        assert call(**bad) == -1, bad


def test_validation_grid_is_one_row_of_eight(tmp_path):
    """reference ValidateNaturalInference.py:236: save_image(samples, path, nrow=8, ...): 8 images -> 1 x 8."""
    import torch
    from PIL import Image
    from naturaldiffusion_amd.ValidateNaturalInference import save_image_grid
    save_image_grid(torch.zeros(8, 3, 16, 16), tmp_path / "g.png")
    assert Image.open(tmp_path / "g.png").size == (8 * 18 + 2, 18 + 2)


def test_png_writer_gives_the_pixels_back(tmp_path):
    """write_png_rgb (the band-parallel deflate of round 5): a reader (PIL) decodes every file to the array it was given -- one band, several bands, ragged band
    heights, a one-pixel image -- and the stream passes PIL's integrity check (CRCs, Adler-32 of the concatenated bands)."""
    import numpy as np
    from PIL import Image
    from naturaldiffusion_amd.ValidateNaturalInference import write_png_rgb, save_image_grid
    import torch
    r = np.random.RandomState(3)
    for shape, threads in (((260, 2066, 3), 8), ((1, 1, 3), 8), ((17, 5, 3), 8), ((300, 33, 3), 3), ((64, 64, 3), 1), ((131, 7, 3), 16)):
        a = r.randint(0, 256, shape).astype(np.uint8)
        if shape[0] > 100:
            a[: shape[0] // 2] = 7                                          # a compressible half: exercises real deflate blocks next to stored ones
        write_png_rgb(a, tmp_path / "a.png", threads=threads)
        Image.open(tmp_path / "a.png").verify()
        assert np.array_equal(np.array(Image.open(tmp_path / "a.png").convert("RGB")), a), (shape, threads)
    with pytest.raises(ValueError):
        write_png_rgb(np.zeros((4, 4), np.uint8), tmp_path / "b.png")
    # through save_image_grid: the values torchvision's save_image(normalize=True, value_range=(-1, 1)) would write
    x = torch.linspace(-1.2, 1.2, 8 * 3 * 16 * 16).reshape(8, 3, 16, 16)
    save_image_grid(x, tmp_path / "g.png")
    got = np.array(Image.open(tmp_path / "g.png").convert("RGB"))
    want = (((x.clamp(-1, 1) + 1) * 0.5) * 255 + 0.5).clamp(0, 255).to(torch.uint8)
    assert np.array_equal(got[2:18, 2:18], want[0].permute(1, 2, 0).numpy()) and np.array_equal(got[2:18, 20:36], want[1].permute(1, 2, 0).numpy())
    assert (got[:2] == 0).all() and (got[:, :2] == 0).all()


def test_generation_pipeline_host_logic(tmp_path):
    """Round 4 host pieces that need no GPU: how `generate_sharded` / `natural_inference_tx` pick their lanes, the reference-statistics argument of the FID
    functions, the FidBlocked result, the handle-sharing ABI's argument checks, the per-workload defaults of bench.py."""
    import ctypes as C
    from naturaldiffusion_amd import CIFAR10NaturalInference as M
    from naturaldiffusion_amd._lib import lib
    f, g = (lambda x, t: x), (lambda x, t: -x)
    assert M._lane_models([f, g], 2, 10) == [f, g]                         # a sequence: one lane each, as given
    assert M._lane_models(f, 2, 10) == [f]                                  # an opaque callable owns state we cannot duplicate: one lane
    mu, sg = np.zeros(4), np.eye(4)
    a, b = M._ref_statistics((mu, sg))
    assert a is not None and np.array_equal(b, sg)
    np.savez(tmp_path / "ref.npz", mu=mu + 1, sigma=2 * sg)
    a, b = M._ref_statistics(tmp_path / "ref.npz")
    assert np.array_equal(a, mu + 1) and np.array_equal(b, 2 * sg)
    with pytest.raises(FileNotFoundError, match="fid: blocked"):
        M._ref_statistics(tmp_path / "absent.npz")
    fb = M.FidBlocked(torch.zeros(3, 32, 32, 3, dtype=torch.uint8), "fid: blocked -- test")
    assert tuple(fb.images.shape) == (3, 32, 32, 3) and "blocked" in fb.reason and "FidBlocked" in repr(fb)
    # natinf_ncsnpp_share: host-side argument / state checks (no GPU involved)
    h1, h2, h3 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.natinf_ncsnpp_create(C.byref(h1), 0) == 0 and lib.natinf_ncsnpp_create(C.byref(h2), 0) == 0 and lib.natinf_ncsnpp_create(C.byref(h3), 2) == 0
    assert lib.natinf_ncsnpp_share(h2, h1) == -4                            # NATINF_ESTATE: nothing loaded into h1
    assert lib.natinf_ncsnpp_share(h1, h1) == -1 and lib.natinf_ncsnpp_share(None, h1) == -1      # NATINF_EINVAL
    for h in (h1, h2, h3):
        lib.natinf_ncsnpp_destroy(h)
    assert lib.natinf_set_flash_mode(7) == -1 and lib.natinf_set_flash_mode(3) == 0 and lib.natinf_set_flash_mode(0) == 0 and lib.natinf_set_flash_mode(3) == 0
    assert lib.natinf_set_flash_mode(1) in (0, -4) and lib.natinf_set_flash_mode(3) == 0           # intermediate forms: retired


def test_bench_line_stays_small(repo_root):
    """the default line must survive a 3 KB log tail: the committed line of the round's final run is the check (bench.py moved every explanation to its docstring)"""
    import json
    f = repo_root / "profiles" / "r04" / "final_bench.json"
    line = f.read_text().strip()
    assert len(line) <= 3072, len(line)
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(d["roofline"]) and set(("value", "unit", "cores", "kind", "sample")) <= set(d["cpu_baseline"])
    assert list(d)[:14][-2:] == ["single_stream", "pipeline"] or "single_stream" in list(d)[:16]       # the like-for-like figure sits with the headline, in front of the sub-objects
    for k in ("sd3", "sd3_fp8", "fid50k", "validate"):
        assert "value" in d[k], k
