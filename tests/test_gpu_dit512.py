"""DiT at 512x512 (input size 64, 1,024 tokens): the streaming attention kernel alone against an fp32 softmax, the engine
against the CPU oracle at that size, and the Validate script end to end with a 64x64 latent."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 3e-2          # max |engine - oracle| / max |oracle| (tests/test_gpu_dit.py)
ATTN_TOL = 1e-2     # max |kernel - fp32 softmax| / max |fp32 softmax|


def _qkv(B, T, H, hd, seed, spike=None):
    """one [B*T][3*H*hd] bf16 buffer (q | k | v, as the engine's GEMM writes it); spike: a key index whose logit is +30 for every query"""
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    x = torch.randn(B, T, 3, H, hd, generator=g)
    if spike is not None:
        x[:, :, 0, :, 0] = 1.0                                        # q channel 0 = 1, k channel 0 = 0 except at the spiked key
        x[:, :, 1, :, 0] = 0.0
        x[:, spike, 1, :, 0] = 30.0 * hd ** 0.5
    return x.reshape(B * T, 3 * D).to(torch.bfloat16).cuda(), D


def _ref(qkv, B, T, H, hd):
    x = qkv.float().reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)      # [3][B][H][T][hd]
    s = torch.softmax(x[0] @ x[1].transpose(-1, -2) * hd ** -0.5, dim=-1)
    return (s @ x[2]).permute(0, 2, 1, 3).reshape(B * T, H * hd)


def _attn(qkv, D, B, T, H, hd, flags=0):
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    o = torch.full((B * T, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    base = ptr(qkv)
    check(lib.natinf_dit_attention_bf16(base, base + 2 * D, base + 4 * D, 3 * D, ptr(o), D, B, T, H, hd, flags, stream_ptr()),
          "natinf_dit_attention_bf16")
    torch.cuda.synchronize()
    return o.float()


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("hd", [64, 72, 96])
@pytest.mark.parametrize("T", [256, 512, 1024])
def test_streaming_attention_matches_fp32_softmax(T, hd):
    B, H = 2, 2
    qkv, D = _qkv(B, T, H, hd, seed=T + hd)
    out = _attn(qkv, D, B, T, H, hd)
    assert torch.isfinite(out).all()
    err = _rel(out, _ref(qkv, B, T, H, hd))
    assert err <= ATTN_TOL, err
    if T == 256:                                                       # the LDS-resident kernel the 256-token engine runs
        res = _attn(qkv, D, B, T, H, hd, flags=1)
        assert _rel(out, res) <= ATTN_TOL


@pytest.mark.parametrize("hd", [72, 64])
def test_streaming_attention_rescales_on_a_late_large_logit(hd):
    """one key 30 logits above the rest, in the 12th of 16 key tiles: every query's running maximum jumps there"""
    B, T, H = 2, 1024, 2
    qkv, D = _qkv(B, T, H, hd, seed=5, spike=739)
    out = _attn(qkv, D, B, T, H, hd)
    ref = _ref(qkv, B, T, H, hd)
    assert torch.isfinite(out).all()
    assert _rel(out, ref) <= ATTN_TOL
    v = qkv.float().reshape(B, T, 3, H * hd)[:, 739, 2]                # the output is (almost) that key's value row
    assert _rel(out.reshape(B, T, H * hd)[:, 0], v) <= ATTN_TOL


def _engine(P, depth, hid, heads, max_batch, **kw):
    from naturaldiffusion_amd.dit import DiTEngine, flatten_state_dict
    return DiTEngine(flatten_state_dict(P, depth, hid), max_batch=max_batch, depth=depth, hidden=hid, heads=heads, input_size=64, **kw)


@pytest.mark.parametrize("depth,hid,heads", [(2, 128, 2), (1, 576, 8)])
def test_small_configs_at_input_64_match_oracle(depth, hid, heads):
    from oracle import dit_oracle as D
    P = D.make_params(depth, hid, seed=7, grid=32)
    g = torch.Generator().manual_seed(depth + hid)
    x, t, y = torch.randn(2, 4, 64, 64, generator=g), torch.tensor([900.0, 20.0]), torch.tensor([207, 1000])
    ref = D.forward(P, x, t, y, heads)
    for unfused in (False, True):
        out = _engine(P, depth, hid, heads, 2, unfused_attention=unfused)(x.cuda(), t.cuda(), y.cuda()).cpu()
        assert out.shape == (2, 8, 64, 64)
        err = _rel(out, ref)
        assert err <= TOL, (unfused, err)


def test_xl2_at_input_64_matches_oracle_fused_unfused_and_both_streams():
    from oracle import dit_oracle as D
    P = D.make_params(28, 1152, seed=3, grid=32)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 64, 64, generator=g)
    t, y = torch.tensor([999.0, 3.0]), torch.tensor([1000, 207])
    ref = D.forward(P, x, t, y, 16)
    eng = _engine(P, 28, 1152, 16, 4)
    out = eng(x.cuda(), t.cuda(), y.cuda()).cpu()
    assert _rel(out, ref) <= TOL
    # a sample's output does not depend on the rest of the batch, nor on its position
    xb = torch.cat([torch.randn(3, 4, 64, 64, generator=g), x[1:2]]).cuda()
    out4 = eng(xb, torch.tensor([77.0, 500.0, 1.0, 3.0]).cuda(), torch.tensor([3, 4, 5, 207]).cuda()).cpu()
    assert (out4[3] - out[1]).abs().max().item() <= 1e-2 * ref.abs().max().item()
    del eng
    unf = _engine(P, 28, 1152, 16, 2, unfused_attention=True)(x.cuda(), t.cuda(), y.cuda()).cpu()
    assert _rel(unf, ref) <= TOL and _rel(out, unf) <= TOL
    f32 = _engine(P, 28, 1152, 16, 2, stream16=False)(x.cuda(), t.cuda(), y.cuda()).cpu()
    h16 = _engine(P, 28, 1152, 16, 2, stream16=True)(x.cuda(), t.cuda(), y.cuda()).cpu()
    assert _rel(f32, ref) <= TOL and _rel(h16, ref) <= TOL


def test_create_sized_32_is_byte_identical_to_create():
    from oracle import dit_oracle as D
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    from naturaldiffusion_amd.dit import DiTEngine, flatten_state_dict
    P = D.make_params(2, 128, seed=9)
    flat = flatten_state_dict(P, 2, 128)
    g = torch.Generator().manual_seed(2)
    x, t, y = torch.randn(2, 4, 32, 32, generator=g).cuda(), torch.tensor([400.0, 7.0]).cuda(), torch.tensor([1, 1000], dtype=torch.int32).cuda()
    sized = DiTEngine(flat, max_batch=2, depth=2, hidden=128, heads=2, input_size=32)(x, t, y)
    h = C.c_void_p()
    check(lib.natinf_dit_create(C.byref(h), 2, 128, 2, 0), "natinf_dit_create")
    try:
        assert lib.natinf_dit_input_size(h) == 32
        params = flat.cuda()
        packed = torch.empty(lib.natinf_dit_packed_bytes(h), dtype=torch.uint8, device="cuda")
        check(lib.natinf_dit_load(h, ptr(params), params.numel(), ptr(packed), packed.numel(), stream_ptr()), "natinf_dit_load")
        ws = torch.empty(lib.natinf_dit_workspace_bytes(h, 2), dtype=torch.uint8, device="cuda")
        out = torch.empty_like(sized)
        check(lib.natinf_dit_forward(h, ptr(x), ptr(t), ptr(y), ptr(out), 2, ptr(ws), ws.numel(), stream_ptr()), "natinf_dit_forward")
        torch.cuda.synchronize()
    finally:
        lib.natinf_dit_destroy(h)
    assert torch.equal(out.view(torch.int32), sized.view(torch.int32))


def test_validate_at_512_original_vs_natural_and_one_decode(tmp_path, monkeypatch):
    """test_gpu_dit.py's DDIM-against-Natural-Inference check with a 64x64-latent engine built from a fresh 512 state dict
    (input size inferred from its pos_embed), then the VAE engine at latent_res 64 writes the 1 x 8 row of 512x512 images."""
    import shutil
    from PIL import Image
    from oracle import vae_oracle as VO
    from naturaldiffusion_amd import ValidateNaturalInference as V
    from naturaldiffusion_amd.dit import DiTEngine, flatten_state_dict, input_size_of
    from naturaldiffusion_amd.synth import synthetic_dit_state_dict
    from safetensors.torch import save_file
    sd = synthetic_dit_state_dict(2, 128, seed=11, input_size=64)
    assert input_size_of(sd) == 64
    eng = DiTEngine(flatten_state_dict(sd, 2, 128), max_batch=16, depth=2, hidden=128, heads=2, input_size=input_size_of(sd))
    monkeypatch.setattr(V, "denoiser_factory", lambda: eng)
    monkeypatch.setattr(V, "device", "cuda:0")
    monkeypatch.setattr(V, "root_path", tmp_path)
    (tmp_path / "results" / "ddim").mkdir(parents=True)
    shutil.copy(V.__file__.rsplit("/", 2)[0] + "/results/ddim/ddim_024.npz", tmp_path / "results" / "ddim" / "ddim_024.npz")
    a = V.ddim_skip_sample(24).clone()
    b = V.natural_inference("ddim", 24)
    assert a.shape == b.shape == (8, 4, 64, 64)
    rel = ((a - b).abs().max() / a.abs().max()).item()
    assert rel < 5e-3, rel
    P = VO.make_params(4, seed=1)
    vsd = {"decoder." + k: v.contiguous() for k, v in P.items()}
    vsd["post_quant_conv.weight"] = torch.eye(4).reshape(4, 4, 1, 1).contiguous()
    vsd["post_quant_conv.bias"] = torch.zeros(4)
    (tmp_path / "vae").mkdir()
    save_file(vsd, str(tmp_path / "vae" / "diffusion_pytorch_model.safetensors"))
    monkeypatch.setattr(V, "vae_path", str(tmp_path / "vae"))
    V._finish(b, "ddim_024__seed_0__natural.png")
    img = Image.open(tmp_path / "results" / "validation" / "ddim_024__seed_0__natural__512x512.png")
    assert img.size == (8 * 514 + 2, 514 + 2)
    assert not (tmp_path / "results" / "validation" / "ddim_024__seed_0__natural.png").exists()
