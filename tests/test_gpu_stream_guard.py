"""The stream guard of the transformer engines on the GPU (include/natinf_dit.h, NATINF_DIT_STREAM_GUARD / NATINF_MMDIT_STREAM_GUARD): inert in range (the guarded
engine writes the unguarded engine's bytes), the monitor agrees with the stream, an overflow is clamped, counted and located, the status block accumulates and
resets, and ``generate_sharded(stream16="auto")`` falls back to the fp32 stream exactly when the half stream was not enough.

Weights: the oracle's synthetic DiT / MMDiT parameters (``make_params``), as in tests/test_gpu_dit.py and tests/test_gpu_mmdit.py.  The overflowing set is the same with
two edits in the LAST block: the MLP branch's adaLN gate is exactly 1 (its rows of the modulation matrix zeroed, their bias 1) and ``mlp.fc2.bias`` of one channel is
2e5 -- so the MLP update of that block writes ~2e5 into one channel of every token (site 2 * depth, the last), everything before it stays O(1-10), and the final
LayerNorm maps the row back to O(sqrt(hidden)): the fp32-stream output is finite.  An inf in a tensor is data; nothing here faults."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 3e-2            # tests/test_gpu_dit.py: max |engine - oracle| / max |oracle|
STREAMS_REL = 5e-3    # tests/test_gpu_dit.py::test_xl2_half_stream_against_the_fp32_stream: half stream against fp32 stream
HALF_MAX = 65504.0
SMALL = dict(depth=3, hidden=256, heads=4)      # hidden % 128 == 0: fp8 applies
BIG_CH = 37


_made = {}


def dit_params(depth, hidden, seed, overflow=False, grid=16):
    from oracle import dit_oracle as D
    key = (depth, hidden, seed, grid)
    if key not in _made:                                        # (DiT-XL/2's 675 M synthetic parameters are drawn once per session)
        _made.clear()
        _made[key] = D.make_params(depth, hidden, seed=seed, grid=grid)
    P = dict(_made[key])
    if overflow:
        p = f"blocks.{depth - 1}."
        for k in ("adaLN_modulation.1.weight", "adaLN_modulation.1.bias", "mlp.fc2.bias"):
            P[p + k] = P[p + k].clone()
        P[p + "adaLN_modulation.1.weight"][5 * hidden:] = 0.0
        P[p + "adaLN_modulation.1.bias"][5 * hidden:] = 1.0
        P[p + "mlp.fc2.bias"][BIG_CH] = 2.0e5
    return P


def dit_engine(P, max_batch, cfg=SMALL, **kw):
    from naturaldiffusion_amd.dit import DiTEngine, flatten_state_dict
    return DiTEngine(flatten_state_dict(P, cfg["depth"], cfg["hidden"]), max_batch=max_batch, **cfg, **kw)


def dit_inputs(n, S=32, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 4, S, S, generator=g).cuda(), torch.linspace(999.0, 3.0, n).cuda(), ((torch.arange(n) * 61) % 1001).cuda())


def show(tag, st):
    print(f"{tag}: max_abs {np.array2string(st['max_abs'], precision=4)} clamped {st['clamped'].tolist()}")


def in_range(st, sites):
    assert st["max_abs"].shape == (sites,) and st["max_abs"].dtype == np.float32 and st["clamped"].shape == (sites,) and st["clamped"].dtype == np.uint32
    assert not st["clamped"].any(), st["clamped"]
    assert np.isfinite(st["max_abs"]).all() and (st["max_abs"] > 0).all() and (st["max_abs"] < HALF_MAX).all(), st["max_abs"]


# ------------------------------------------------------------------------------ 1. inert in range
@pytest.mark.parametrize("unfused", [False, True], ids=["fused", "unfused"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("s16", [True, False], ids=["half", "fp32"])
def test_small_dit_guard_is_inert_in_range(s16, fp8, unfused):
    P = dit_params(seed=7, **{k: SMALL[k] for k in ("depth", "hidden")})
    x, t, y = dit_inputs(5)
    plain = dit_engine(P, 6, stream16=s16, fp8=fp8, unfused_attention=unfused)
    guarded = dit_engine(P, 6, stream16=s16, fp8=fp8, unfused_attention=unfused, guard=True)
    assert guarded.site_names == ["patch_embed"] + [f"blocks.{i}.{b}" for i in range(3) for b in ("attn", "mlp")]
    assert guarded.workspace_bytes >= plain.workspace_bytes + 8 * 7
    a, b = plain(x, t, y), guarded(x, t, y)
    assert torch.isfinite(a).all() and torch.equal(a, b), "in range the guarded engine must write the unguarded engine's bytes"
    st = guarded.stream_status()
    show(f"small DiT s16={s16} fp8={fp8} unfused={unfused}", st)
    in_range(st, 7)
    with pytest.raises(RuntimeError):
        plain.stream_status()


@pytest.mark.parametrize("S", [32, 64])
def test_small_dit_both_input_sizes(S):
    P = dit_params(2, 128, seed=11, grid=S // 2)
    cfg = dict(depth=2, hidden=128, heads=2)
    x, t, y = dit_inputs(3, S)
    a = dit_engine(P, 4, cfg, input_size=S)(x, t, y)
    g = dit_engine(P, 4, cfg, input_size=S, guard=True)
    assert torch.equal(a, g(x, t, y))
    in_range(g.stream_status(), 5)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_xl2_guard_is_inert_in_range(fp8):
    """DiT-XL/2 at the Validate script's forward of 16: the four-wave tile's guarded epilogue (16-byte half form) and the guarded split-K reduce behind fc2."""
    from naturaldiffusion_amd.dit import XL2
    P = dit_params(28, 1152, seed=3)
    x, t, y = dit_inputs(16)
    outs = {}
    for s16 in (True, False):
        a = dit_engine(P, 16, XL2, stream16=s16, fp8=fp8)(x, t, y)
        g = dit_engine(P, 16, XL2, stream16=s16, fp8=fp8, guard=True)
        b = g(x, t, y)
        assert torch.isfinite(a).all() and torch.equal(a, b), f"stream16={s16}"
        st = g.stream_status()
        print(f"DiT-XL/2 fp8={fp8} stream16={s16}: max_abs over the sites {st['max_abs'].min():.3f} .. {st['max_abs'].max():.3f}")
        in_range(st, 57)
        outs[s16] = st
        del g
    # the two streams see the same stream: the bound the two engines' outputs are held to
    rel = np.abs(outs[True]["max_abs"] - outs[False]["max_abs"]).max() / outs[False]["max_abs"].max()
    assert rel <= STREAMS_REL, rel


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("s16", [True, False], ids=["half", "fp32"])
def test_mmdit_guard_is_inert_in_range(s16, fp8):
    from oracle import mmdit_oracle as M
    from naturaldiffusion_amd.mmdit import MMDiTEngine, flatten_state_dict
    cfg = dict(layers=3, heads=2, joint_dim=64, pooled_dim=32)                       # the reduced size of tests/test_gpu_mmdit.py
    P = M.make_params(seed=4, pos_max=24, pos_base=8, **cfg)
    flat = flatten_state_dict(P, 8, **cfg)
    g = torch.Generator().manual_seed(0)
    x, t = torch.randn(3, 16, 16, 16, generator=g).cuda(), torch.tensor([900.0, 10.0, 455.5]).cuda()
    e, p = torch.randn(3, 13, 64, generator=g).cuda(), torch.randn(3, 32, generator=g).cuda()
    kw = dict(max_batch=4, grid=8, ctx_tokens=13, fp8=fp8, stream16=s16, **cfg)
    plain, guarded = MMDiTEngine(flat, **kw), MMDiTEngine(flat, guard=True, **kw)
    assert guarded.site_names == ["patch_embed"] + [f"blocks.{i}.{b}" for i in range(3) for b in ("attn", "mlp")]
    a, b = plain.forward(x, t, e, p), guarded.forward(x, t, e, p)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    st = guarded.stream_status()
    show(f"MMDiT s16={s16} fp8={fp8}", st)
    in_range(st, 7)
    # accumulation and reset, as for the DiT engine
    guarded.forward(x, t, e, p)
    st2 = guarded.stream_status()
    assert np.array_equal(st2["max_abs"], st["max_abs"]) and not st2["clamped"].any()
    guarded.reset_stream_status()
    z = guarded.stream_status()
    assert not z["max_abs"].any() and not z["clamped"].any()


# ------------------------------------------------------------------------------ 2. the monitor agrees with the stream
def test_monitor_agrees_with_the_oracles_stream():
    from oracle import dit_oracle as D
    P = dit_params(seed=7, **{k: SMALL[k] for k in ("depth", "hidden")})
    x, t, y = dit_inputs(5)
    taps = {}
    D.forward(P, x.cpu(), t.cpu(), y.cpu(), SMALL["heads"], taps=taps)
    final = float(taps["block2"].abs().max())
    embed = float(taps["embed"].abs().max())
    g = dit_engine(P, 6, stream16=False, guard=True)                                 # fused attention: NATINF_DIT_UNFUSED_ATTENTION off
    g(x, t, y)
    st = g.stream_status()
    show("fp32-stream monitor", st)
    print(f"oracle: max |embedding| {embed:.4f}, max |final stream| {final:.4f}")
    assert st["max_abs"][-1] >= final * (1 - TOL), (st["max_abs"][-1], final)
    assert st["max_abs"][0] >= embed * (1 - TOL), (st["max_abs"][0], embed)
    # monotone under accumulation: other inputs never lower it, and the same inputs leave it where it is
    x2, t2, y2 = dit_inputs(6, seed=9)
    g(x2 * 0.5, t2, y2)
    st2 = g.stream_status()
    assert (st2["max_abs"] >= st["max_abs"]).all() and not st2["clamped"].any()
    g(x, t, y)
    assert np.array_equal(g.stream_status()["max_abs"], st2["max_abs"])


# ------------------------------------------------------------------------------ 3. overflow is caught and located
@pytest.mark.parametrize("case", ["small_bf16", "small_fp8", "small_unfused", "xl2_bf16", "xl2_fp8"])
def test_overflow_is_clamped_counted_and_located(case):
    from naturaldiffusion_amd.dit import XL2
    size, mode = case.split("_")
    cfg = SMALL if size == "small" else XL2
    n = 5 if size == "small" else 16                                                 # XL/2 at 16: the MLP update goes through the split-K reduce
    P = dit_params(cfg["depth"], cfg["hidden"], seed=7, overflow=True)
    kw = dict(fp8=mode == "fp8", unfused_attention=mode == "unfused")
    x, t, y = dit_inputs(n)
    last = 2 * cfg["depth"]
    # preconditions, on the fp32-stream guarded engine (the measuring instrument)
    wide = dit_engine(P, n, cfg, stream16=False, guard=True, **kw)
    out32 = wide(x, t, y)
    st32 = wide.stream_status()
    show(f"{case} fp32 stream", st32)
    assert torch.isfinite(out32).all()
    assert st32["max_abs"][last] > 1e5, st32["max_abs"][last]
    assert (st32["max_abs"][:last] < HALF_MAX).all(), st32["max_abs"][:last]
    assert not st32["clamped"].any(), "an fp32 stream is tracked, never clamped"
    del wide
    # the guarded half stream
    half = dit_engine(P, n, cfg, stream16=True, guard=True, **kw)
    out16 = half(x, t, y)
    st16 = half.stream_status()
    show(f"{case} half stream", st16)
    assert torch.isfinite(out16).all(), "the guarded half stream must not turn the overflow into inf / NaN"
    assert st16["clamped"][last] > 0 and not st16["clamped"][:last].any(), st16["clamped"]
    assert st16["clamped"][last] == n * 256, "one channel of every token left the half range"
    rel = abs(float(st16["max_abs"][last]) - float(st32["max_abs"][last])) / float(st32["max_abs"][last])
    assert rel <= STREAMS_REL, (st16["max_abs"][last], st32["max_abs"][last])
    assert (st16["max_abs"][:last] < HALF_MAX).all()


def test_nan_reads_back_as_nan():
    """A NaN update is data too: it stays NaN in the stream, is counted, and max_abs of its site reads back as NaN (its bit pattern sorts above inf)."""
    P = dit_params(2, 128, seed=11)
    P["blocks.0.attn.proj.bias"] = P["blocks.0.attn.proj.bias"].clone()
    P["blocks.0.attn.proj.bias"][5] = float("nan")
    cfg = dict(depth=2, hidden=128, heads=2)
    x, t, y = dit_inputs(2)
    for s16 in (True, False):
        g = dit_engine(P, 2, cfg, stream16=s16, guard=True)
        out = g(x, t, y)
        st = g.stream_status()
        assert np.isfinite(st["max_abs"][0]) and np.isnan(st["max_abs"][1:]).all(), st["max_abs"]
        assert torch.isnan(out).any()
        assert (st["clamped"][1:] > 0).all() if s16 else not st["clamped"].any()


# ------------------------------------------------------------------------------ 4. reset and accumulation
def test_reset_accumulation_and_workspace_independence():
    P = dit_params(SMALL["depth"], SMALL["hidden"], seed=7, overflow=True)
    xa, ta, ya = dit_inputs(5)
    xb, tb, yb = dit_inputs(3, seed=21)
    g = dit_engine(P, 6, stream16=True, guard=True)
    g.reset_stream_status()
    z = g.stream_status()
    assert not z["max_abs"].any() and not z["clamped"].any()                         # all zero after a reset
    g(xa, ta, ya)
    a = g.stream_status()
    g.reset_stream_status()
    g(xb, tb, yb)
    b = g.stream_status()
    g.reset_stream_status()
    g(xa, ta, ya)
    g(xb, tb, yb)
    ab = g.stream_status()
    assert np.array_equal(ab["clamped"], a["clamped"] + b["clamped"]) and ab["clamped"][-1] == 8 * 256
    assert np.array_equal(ab["max_abs"], np.maximum(a["max_abs"], b["max_abs"]))
    # the status is a property of the forward, not of the workspace it ran in: a second workspace holding other bytes gives the same figures
    ws1 = g._ws
    g._ws = torch.full_like(ws1, 0x5A)
    g.reset_stream_status()
    out2 = g(xa, ta, ya)
    a2 = g.stream_status()
    g._ws = ws1
    g.reset_stream_status()
    assert torch.equal(out2, g(xa, ta, ya))
    assert np.array_equal(a2["max_abs"], a["max_abs"]) and np.array_equal(a2["clamped"], a["clamped"])
    assert np.array_equal(g.stream_status()["clamped"], a["clamped"])


# ------------------------------------------------------------------------------ 5. the job
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_job_auto_falls_back_exactly_when_needed(fp8):
    from naturaldiffusion_amd import ValidateNaturalInference as V
    kw = dict(alg_name="ddpm_sympy", num_step=24, batch_size=2, seed=3, decode=False)
    labels = [(91 * i + 7) % 1000 for i in range(5)]
    for overflow in (True, False):
        P = dit_params(SMALL["depth"], SMALL["hidden"], seed=13, overflow=overflow)
        half = dit_engine(P, 4, stream16=True, fp8=fp8)
        wide = dit_engine(P, 4, stream16=False, fp8=fp8)
        guarded = dit_engine(P, 4, stream16=True, fp8=fp8, guard=True)
        made, report = [], {}
        z, lb, ix, _ = V.generate_sharded(5, labels, model=guarded, stream16="auto", fallback=lambda: (made.append(1), wide)[1], report=report, **kw)
        print(f"overflow={overflow} fp8={fp8}: report {report}")
        assert ix.tolist() == list(range(5)) and lb.tolist() == labels
        if overflow:
            ref = V.generate_sharded(5, labels, model=wide, stream16=False, **kw)[0]
            assert torch.isfinite(ref).all() and torch.equal(z, ref), "every batch overflows: the job must return the fp32-stream job's latents"
            assert report["rerun_batches"] == [0, 1, 2] and report["batches"] == 3 and len(made) == 1
            fc = report["first_clamp"]
            assert fc["batch"] == 0 and fc["site"] == 2 * SMALL["depth"] and fc["site_name"] == "blocks.2.mlp" and fc["max_abs"] > 1e5 and fc["clamped"] > 0
        else:
            ref = V.generate_sharded(5, labels, model=half, stream16=True, **kw)[0]
            assert torch.equal(z, ref), "in range the job must return the half-stream job's bytes"
            assert report == dict(batches=3, rerun_batches=[], first_clamp=None) and not made
        # two calls over the image range give the same images (single-image batches: each image's forward has the same shape in both splits)
        k1 = dict(kw, batch_size=1)
        rep = {}
        whole = V.generate_sharded(4, labels[:4], model=guarded, stream16="auto", fallback=lambda: wide, report=rep, **k1)[0]
        assert rep["rerun_batches"] == ([0, 1, 2, 3] if overflow else [])
        full = torch.empty_like(whole)
        for r in range(2):
            zz, _, ii, _ = V.generate_sharded(4, labels[:4], model=guarded, stream16="auto", fallback=lambda: wide, rank=r, world=2, **k1)
            full[ii.cuda()] = zz
        assert torch.equal(full, whole)
        del half, wide, guarded
