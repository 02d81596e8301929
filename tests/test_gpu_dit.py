"""HIP DiT engine (include/natinf_dit.h) against the CPU oracle (oracle/dit_oracle.py, pinned to the reference's
DiT class by tests/golden/dit_forward.npz).  bf16 operands / fp32 accumulation against an fp32 oracle: tolerance is
relative to the output's max magnitude, as for the NCSN++ engine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 3e-2          # max |engine - oracle| / max |oracle|


def _flat(P, depth, hid):
    from naturaldiffusion_amd.dit import flatten_state_dict
    return flatten_state_dict(P, depth, hid)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(golden_dir / "dit_forward.npz")


@pytest.mark.parametrize("unfused", [False, True])
@pytest.mark.parametrize("tag,depth,hid,heads", [("s64", 2, 128, 2), ("s72", 1, 576, 8)])
def test_small_configs_match_golden(fx, tag, depth, hid, heads, unfused):
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.dit import DiTEngine
    P = D.make_params(depth, hid, seed=7)
    eng = DiTEngine(_flat(P, depth, hid), max_batch=4, depth=depth, hidden=hid, heads=heads, unfused_attention=unfused)
    x, t, y = (torch.from_numpy(fx[f"{tag}_{k}"]) for k in ("x", "t", "y"))
    out = eng(x.cuda(), t.cuda(), y.cuda()).cpu().numpy()
    ref = fx[f"{tag}_out"]
    assert out.shape == ref.shape
    err = np.abs(out - ref).max() / np.abs(ref).max()
    assert err <= TOL, err


def test_xl2_matches_oracle_and_batch_independent():
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.dit import DiTEngine
    P = D.make_params(28, 1152, seed=3)
    eng = DiTEngine(_flat(P, 28, 1152), max_batch=8)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 4, 32, 32, generator=g)
    t = torch.tensor([999.0, 500.0, 3.0])
    y = torch.tensor([1000, 207, 0])
    ref = D.forward(P, x, t, y, 16).numpy()
    out = eng(x.cuda(), t.cuda(), y.cuda()).cpu().numpy()
    err = np.abs(out - ref).max() / np.abs(ref).max()
    assert err <= TOL, err
    # a sample's output does not depend on what else is in the batch, nor on its position
    xb = torch.cat([x[2:3], torch.randn(5, 4, 32, 32, generator=g)]).cuda()
    tb = torch.cat([t[2:3], torch.full((5,), 77.0)]).cuda()
    yb = torch.cat([y[2:3], torch.tensor([3, 4, 5, 6, 7])]).cuda()
    out8 = eng(xb, tb, yb).cpu().numpy()
    assert np.abs(out8[0] - out[2]).max() <= 1e-2 * np.abs(ref).max()


def test_xl2_half_stream_against_the_fp32_stream():
    """natinf_set_dit_stream16 (round 6; the library's default): the residual stream in IEEE half against the fp32 stream at DiT-XL/2 size -- the direct residual
    epilogue on 128 x 128 tiles (its 16-byte form: v_permlane16_swap) and behind the split-K reduce pass, k_ln_modulate_v4<4, 128, true, RowsBf16>, k_patch_embed<true, false> (csrc/transformer_rows.h) --:
    both inside the oracle bound, close to each other, and the stream is the only buffer that shrinks."""
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.dit import DiTEngine
    P = D.make_params(28, 1152, seed=3)
    flat = _flat(P, 28, 1152)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(16, 4, 32, 32, generator=g)                      # the Validate script's forward of 16: fc2 takes the split-K path there
    t = torch.linspace(999.0, 3.0, 16)
    y = torch.arange(16) * 60
    ref = D.forward(P, x[:2], t[:2], y[:2], 16).numpy()
    outs, ws = {}, {}
    for s16 in (False, True):
        eng = DiTEngine(flat, max_batch=16, stream16=s16)
        outs[s16] = eng(x.cuda(), t.cuda(), y.cuda()).cpu().numpy()
        ws[s16] = eng.workspace_bytes
        del eng
    assert ws[True] == ws[False] - 16 * 256 * 1152 * 2
    for s16 in (False, True):
        err = np.abs(outs[s16][:2] - ref).max() / np.abs(ref).max()
        print(f"DiT-XL/2 stream16={s16}: max rel err against the oracle {err:.3e}")
        assert np.isfinite(outs[s16]).all() and err <= TOL, (s16, err)
    d = np.abs(outs[True] - outs[False]).max() / np.abs(outs[False]).max()
    print(f"half stream against fp32 stream: {d:.3e}")
    assert d <= 5e-3, d


@pytest.mark.parametrize("hid,heads", [(128, 2), (576, 8), (192, 2), (768, 8)])      # head_dim 64, 72, 96 (fused) and 96
def test_fused_attention_equals_per_head_path(hid, heads):
    """One block: the fused attention launch against the per-head GEMM / softmax / GEMM path on the same weights.  Both
    round P to bf16 (the fused kernel before, the other after the 1/sum), so they agree to bf16 resolution."""
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.dit import DiTEngine
    P = D.make_params(1, hid, seed=2)
    flat = _flat(P, 1, hid)
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(3, 4, 32, 32, generator=g) * 2).cuda()
    t = torch.tensor([10.0, 400.0, 900.0]).cuda()
    y = torch.tensor([1, 2, 1000]).cuda()
    a = DiTEngine(flat, 3, depth=1, hidden=hid, heads=heads)(x, t, y)
    b = DiTEngine(flat, 3, depth=1, hidden=hid, heads=heads, unfused_attention=True)(x, t, y)
    ref = D.forward(P, x.cpu(), t.cpu(), y.cpu(), heads)
    assert ((a - b).abs().max() / b.abs().max()).item() <= 1e-2
    assert ((a.cpu() - ref).abs().max() / ref.abs().max()).item() <= TOL


def test_argument_errors():
    from oracle import dit_oracle as D
    from naturaldiffusion_amd.dit import DiTEngine
    P = D.make_params(1, 128, seed=1)
    with pytest.raises(ValueError):
        DiTEngine(_flat(P, 1, 128)[:-1], max_batch=2, depth=1, hidden=128, heads=2)
    eng = DiTEngine(_flat(P, 1, 128), max_batch=2, depth=1, hidden=128, heads=2)
    with pytest.raises(ValueError):
        eng(torch.zeros(3, 4, 32, 32).cuda(), torch.zeros(3), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        DiTEngine(_flat(P, 1, 128), max_batch=2, depth=1, hidden=100, heads=2)


@pytest.mark.parametrize("max_batch", [8, 16], ids=["two_forwards_of_8", "one_forward_of_16"])
def test_validate_natural_inference_end_to_end(monkeypatch, max_batch):
    """src/ValidateNaturalInference.py:311-372 with the HIP DiT engine as the denoiser (the CFG pair of a step as two forwards of 8 or -- when the
    engine takes 16 samples -- as one forward of [z; z], one fused natinf_step_f32prod launch per step) against the oracle's restatement driven
    by the DiT oracle."""
    from oracle import dit_oracle as D, ni_oracle as O
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd.dit import DiTEngine
    from naturaldiffusion_amd.coeff import load_coeff_npz
    depth, hid, heads = 2, 128, 2
    P = D.make_params(depth, hid, seed=11)
    eng = DiTEngine(_flat(P, depth, hid), max_batch=max_batch, depth=depth, hidden=hid, heads=heads)
    g = torch.Generator().manual_seed(0)
    draws = [torch.randn(8, 4, 32, 32, generator=g) for _ in range(25)]
    it = iter(draws)
    monkeypatch.setattr(V.torch, "randn", lambda *a, **k: next(it).cuda())
    monkeypatch.setattr(V.torch, "randn_like", lambda *a, **k: next(it).cuda())
    monkeypatch.setattr(V, "denoiser_factory", lambda: eng)
    monkeypatch.setattr(V, "device", "cuda:0")
    z = V.natural_inference("ddim", 24).cpu()

    labels = torch.tensor([207, 360, 387, 974, 88, 979, 417, 279])
    nulls = torch.full((8,), 1000)

    def eps_fn(x, t):
        tt = torch.full((8,), float(t))
        c = D.forward(P, x, tt, labels, heads)[:, :4]
        u = D.forward(P, x, tt, nulls, heads)[:, :4]
        return O.cfg_fuse(c, u, 4.0)
    C, B, node = load_coeff_npz(V.root_path / "results/ddim/ddim_024.npz")
    ref = O.validate_ni(eps_fn, draws[0], draws[1:], C, B, node)
    rel = ((z - ref).abs().max() / ref.abs().max()).item()
    assert rel <= 5e-2, rel


def test_original_vs_natural_with_the_bf16_engine(monkeypatch):
    """The reference's own consistency check (src/ValidateNaturalInference.py:375-391: classical DDIM vs its Natural
    Inference form) with the HIP DiT engine as the denoiser.  The two samplers agree to ~4e-7 with a denoiser that is a
    smooth fp32 function (tests/test_gpu_ni_step.py); a bf16-operand denoiser turns 1e-7 input differences into 1e-3
    output differences (one flipped operand rounding), so with it the pair agrees to bf16 resolution, not fp32."""
    from oracle import dit_oracle as D
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd.dit import DiTEngine
    P = D.make_params(2, 128, seed=11)
    eng = DiTEngine(_flat(P, 2, 128), max_batch=8, depth=2, hidden=128, heads=2)
    monkeypatch.setattr(V, "denoiser_factory", lambda: eng)
    monkeypatch.setattr(V, "device", "cuda:0")
    a = V.ddim_skip_sample(24).clone()
    b = V.natural_inference("ddim", 24)
    rel = ((a - b).abs().max() / a.abs().max()).item()
    print("original vs natural, bf16 engine:", rel)
    assert rel < 5e-3, rel          # observed 7.6e-4
