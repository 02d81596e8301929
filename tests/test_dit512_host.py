"""DiT at input size 64 (512x512 images, 1,024 tokens) on the host side: the parameter layout against the oracle, the
state-dict checks, the synthetic position table and the C ABI's argument checks (none of them launches a kernel)."""
import ctypes as C
import math

import pytest
import torch


def test_param_layout_at_input_64_matches_the_oracle():
    from naturaldiffusion_amd.dit import param_layout
    from oracle import dit_oracle as D
    lay = param_layout(28, 1152, input_size=64)
    assert dict(lay)["pos_embed"] == (1, 1024, 1152)
    ref = D.param_shapes(28, 1152, grid=32)
    assert dict(lay) == {k: tuple(v) for k, v in ref.items()}
    assert sum(math.prod(s) for _, s in lay) == sum(math.prod(s) for s in ref.values())
    assert param_layout(28, 1152) == param_layout(28, 1152, input_size=32)
    with pytest.raises(ValueError):
        param_layout(2, 128, input_size=48)


def test_flatten_infers_the_input_size_and_rejects_a_mismatch():
    from naturaldiffusion_amd.dit import flatten_state_dict, input_size_of, param_layout
    from oracle import dit_oracle as D
    P64 = D.make_params(1, 64, seed=1, grid=32)
    P32 = D.make_params(1, 64, seed=1)
    assert input_size_of(P64) == 64 and input_size_of(P32) == 32
    n64 = sum(math.prod(s) for _, s in param_layout(1, 64, 64))
    assert flatten_state_dict(P64, 1, 64).numel() == n64
    assert flatten_state_dict(P64, 1, 64, input_size=64).numel() == n64
    assert flatten_state_dict(P32, 1, 64).numel() == n64 - 768 * 64
    with pytest.raises(ValueError, match="pos_embed"):
        flatten_state_dict(P64, 1, 64, input_size=32)                  # a 1,024-token dict for an input-32 engine
    bad = dict(P32, pos_embed=torch.zeros(1, 100, 64))
    with pytest.raises(ValueError, match="100 tokens"):
        flatten_state_dict(bad, 1, 64)


def test_synthetic_position_table_at_grid_32():
    from naturaldiffusion_amd.synth import synthetic_dit_state_dict
    from oracle import dit_oracle as D
    sd = synthetic_dit_state_dict(1, 64, seed=0, input_size=64)
    assert tuple(sd["pos_embed"].shape) == (1, 1024, 64)
    assert torch.allclose(sd["pos_embed"][0], D.pos_embed_2d(64, 32), atol=1e-6)


def test_create_sized_arguments_and_parameter_count():
    from naturaldiffusion_amd._lib import lib
    for bad in (0, 16, 48, 128):
        assert lib.natinf_dit_create_sized(C.byref(C.c_void_p()), 2, 128, 2, bad, 0) == -1
    h32, h64, h = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.natinf_dit_create_sized(C.byref(h32), 2, 1152, 16, 32, 0) == 0
    assert lib.natinf_dit_create_sized(C.byref(h64), 2, 1152, 16, 64, 1) == 0
    assert lib.natinf_dit_create(C.byref(h), 2, 1152, 16, 0) == 0
    try:
        assert lib.natinf_dit_input_size(h32) == 32 and lib.natinf_dit_input_size(h64) == 64 and lib.natinf_dit_input_size(h) == 32
        assert lib.natinf_dit_input_size(None) == -1
        n32, n64 = lib.natinf_dit_param_count(h32), lib.natinf_dit_param_count(h64)
        assert n64 == n32 + 768 * 1152 and n32 == lib.natinf_dit_param_count(h)
        assert lib.natinf_dit_workspace_bytes(h64, 1) > 4 * lib.natinf_dit_workspace_bytes(h32, 1)
    finally:
        for x in (h32, h64, h):
            lib.natinf_dit_destroy(x)


@pytest.mark.parametrize("T,hd,flags", [(192, 72, 0), (128, 72, 0), (1000, 72, 0), (8192, 72, 0), (1024, 100, 0), (1024, 12, 0),
                                        (1024, 104, 0), (1024, 0, 0), (512, 72, 1), (256, 72, 2)])
def test_attention_entry_rejects_what_it_does_not_support(T, hd, flags):
    """checked before anything touches the device: supported are T % 128 == 0 in [256, 4096], hd % 8 == 0 up to 96
    (the 256-token kernel: T == 256 only)"""
    from naturaldiffusion_amd._lib import lib
    p = 1 << 20                                                        # (never dereferenced)
    ld = max(3 * 2 * max(hd, 8), 8)
    assert lib.natinf_dit_attention_bf16(p, p, p, ld, p, ld, 1, T, 2, hd, flags, None) == -1
