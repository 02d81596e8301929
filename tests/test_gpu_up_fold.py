"""natinf_set_fuse_up_fold: Conv_0 of the 16 -> 32 up-sampling res-block, conv3x3(nearest_up_2x(silu(GroupNorm(x)))), as four 2x2 phase convolutions over the 16x16
tensor (csrc/up_fold.h: k_fold_up_conv, k_conv_gn_upfold; csrc/gemm_dma.h: UPW).  (1) the device fold against its numpy mirror, bit for bit; (2) the launch alone against float64
PyTorch of the unfolded op, with the bounds tests/test_gpu_conv_gn.py::test_up_sampling_fetch_paths_match_torch uses for the nine-tap path (1e-2 of max |ref| on the
output, 5e-3 of max |want| on the GroupNorm partial sums); (3) the engine with the switch on against the switch off.  The tap / parity / border mapping itself is pinned
without a GPU in tests/test_up_fold_host.py."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from up_fold_mirror import fold_up_numpy

pytestmark = pytest.mark.gpu

TOL = 3e-2          # tests/test_gpu_ncsnpp.py: the network output against the reference module


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_device_fold_equals_the_numpy_mirror_bit_for_bit():
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    w = torch.randn(32, 64, 3, 3, generator=torch.Generator().manual_seed(3))
    wd = w.cuda()
    for w_mul in (1.0, -0.6931471805599453):
        out = torch.zeros(2, 2, 32, 64, 2, 2, device="cuda")
        packed = torch.zeros(4 * 32, 4 * 64, dtype=torch.bfloat16, device="cuda")
        check(lib.natinf_debug_fold_up_weights(ptr(wd), 32, 64, w_mul, ptr(out), ptr(packed), stream_ptr()), "fold")
        torch.cuda.synchronize()
        want = fold_up_numpy(w.numpy(), np.float32(w_mul))
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
        # the packed copy: the same values rounded to bf16 once, row (2 a + b) * N + n, column ((c / 64) * 4 + 2 ty + tx) * 64 + c % 64
        wp = torch.from_numpy(want).bfloat16().reshape(4, 32, 1, 64, 4).permute(0, 1, 2, 4, 3).reshape(4 * 32, 4 * 64)
        assert torch.equal(packed.cpu().view(torch.int16), wp.view(torch.int16))


@pytest.fixture(scope="module")
def launch_case():
    """one set of inputs and its float64 reference per (B, cin), shared by the cases below and left unchanged"""
    cache = {}

    def get(B, cin):
        if (B, cin) in cache:
            return cache[(B, cin)]
        N = 256
        g = torch.Generator().manual_seed(1000 * B + cin)
        bf = lambda t: t.bfloat16().float()
        x = bf(torch.randn(B, 16, 16, cin, generator=g))
        scale = torch.rand(B, cin, generator=g) * 1.5 + 0.25
        shift = torch.randn(B, cin, generator=g) * 0.5
        w = bf(torch.randn(N, cin, 3, 3, generator=g) / np.sqrt(9 * cin))
        bias = torch.randn(N, generator=g) * 0.1
        rowvec = torch.randn(B, N, generator=g) * 0.2
        up = lambda t: F.interpolate(t.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
        h = bf(F.silu(x * scale[:, None, None, :] + shift[:, None, None, :]))             # the activated operand is bf16 on the device too
        conv = F.conv2d(up(h).double(), w.double(), padding=1).permute(0, 2, 3, 1)        # [B][32][32][N]
        cache[(B, cin)] = dict(x=x, scale=scale, shift=shift, w=w, bias=bias, rowvec=rowvec, conv=conv)
        return cache[(B, cin)]
    return get


def _run_launch(c, B, cin, use_rowvec, use_parts, out_scale=0.70710678):
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    N, dev = 256, "cuda"
    xd, scd, shd, wd, bd = c["x"].bfloat16().to(dev).contiguous(), c["scale"].to(dev), c["shift"].to(dev), c["w"].to(dev).contiguous(), c["bias"].to(dev)
    rvd = c["rowvec"].to(dev).contiguous() if use_rowvec else None
    wpk = torch.zeros(4 * N, 4 * cin, dtype=torch.bfloat16, device=dev)
    hs = torch.full((B, 18, 18, cin), float("nan"), dtype=torch.bfloat16, device=dev)     # the pass writes its own zero border
    out = torch.full((B * 1024, N), float("nan"), dtype=torch.bfloat16, device=dev)       # every output element must be written
    part = torch.full((4 * B, N // 4, 2), float("nan"), device=dev) if use_parts else None
    check(lib.natinf_debug_conv_up_fold(B, N, cin, ptr(xd), ptr(scd), ptr(shd), ptr(wd), ptr(wpk), ptr(hs), ptr(bd), ptr(rvd), out_scale, ptr(out), ptr(part), 1,
                                        stream_ptr()), "conv_up_fold")
    torch.cuda.synchronize()
    return out.cpu(), (part.cpu() if use_parts else None)


@pytest.mark.parametrize("B,cin", [(1, 64), (3, 64), (1, 128), (3, 128)])           # two and four 64-channel chunks, an odd batch; every border pixel of both parities
@pytest.mark.parametrize("use_rowvec,use_parts", [(True, True), (False, False)])    # the time-embedding row and the GroupNorm partials (epilogue 2), neither (epilogue 1)
def test_up_fold_launch_matches_torch(launch_case, B, cin, use_rowvec, use_parts):
    c = launch_case(B, cin)
    N, out_scale = 256, 0.70710678
    ref = c["conv"] + c["bias"].double()
    if use_rowvec:
        ref = ref + c["rowvec"].double()[:, None, None, :]
    ref = (ref * out_scale).float()                                                   # [B][32][32][N]
    out, part = _run_launch(c, B, cin, use_rowvec, use_parts, out_scale)
    got = out.float().reshape(B, 32, 32, N)
    assert torch.isfinite(got).all()
    err = _rel(got, ref)
    print(f"up-fold launch B={B} cin={cin} rowvec={use_rowvec}: max-rel {err:.3e}")
    assert err <= 1e-2, err
    if use_parts:
        # row 4 s + 2 a + b: (sum, sum of squares) over the 256 pixels (2 i + a, 2 j + b) of sample s, per 4-channel quad
        want = torch.empty(B, 2, 2, N // 4, 2)
        for a in (0, 1):
            for b in (0, 1):
                ph = ref[:, a::2, b::2, :].reshape(B, 256, N // 4, 4)
                want[:, a, b, :, 0] = ph.sum(dim=(1, 3))
                want[:, a, b, :, 1] = (ph ** 2).sum(dim=(1, 3))
        want = want.reshape(4 * B, N // 4, 2)
        perr = _rel(part, want)
        print(f"  GroupNorm partials: max-rel {perr:.3e}")
        assert perr <= 5e-3, perr


def test_a_samples_bytes_do_not_depend_on_its_slot(launch_case):
    """the same image in slots 0 and B - 1 of a batch gives the same bytes (and the same partial sums)"""
    B, cin = 3, 128
    c = dict(launch_case(B, cin))
    for k in ("x", "scale", "shift", "rowvec"):
        t = c[k].clone()
        t[B - 1] = t[0]
        c[k] = t
    out, part = _run_launch(c, B, cin, True, True)
    out = out.view(torch.int16).reshape(B, 1024, 256)
    assert torch.equal(out[0], out[B - 1])
    part = part.reshape(B, 4, 64, 2)
    assert torch.equal(part[0], part[B - 1])


def test_up_fold_argument_errors():
    from naturaldiffusion_amd._lib import lib
    d = 4096
    assert lib.natinf_debug_conv_up_fold(1, 128, 64, d, d, d, d, d, d, None, None, 1.0, d, None, 1, None) == -1      # N: one 256-channel column tile per phase
    assert lib.natinf_debug_conv_up_fold(1, 256, 96, d, d, d, d, d, d, None, None, 1.0, d, None, 1, None) == -1      # cin % 64
    assert lib.natinf_debug_conv_up_fold(1, 256, 64, d, d, d, d, None, d, None, None, 1.0, d, None, 1, None) == -1   # no buffer for the folded weights
    assert lib.natinf_debug_fold_up_weights(d, 32, 48, 1.0, None, d, None) == -1                                        # packed K order: 64-channel chunks


def _describe_gemms(eng, B):
    import ctypes as C
    from naturaldiffusion_amd._lib import lib
    buf = C.create_string_buffer(1 << 16)
    n = lib.natinf_ncsnpp_describe_gemms(eng._h, B, buf, len(buf))
    assert n > 0
    return buf.value.decode().strip().split("\n")


@pytest.fixture(scope="module")
def flat():
    from oracle import ncsnpp_oracle as N
    from naturaldiffusion_amd.ncsnpp import flatten_state_dict
    return flatten_state_dict(N.make_params(seed=0))


@pytest.mark.parametrize("B", [5, 64])
def test_engine_with_the_fold_against_the_plan_without(flat, golden_dir, B):
    """The plan with the switch on against the plan with it off (the 2e-2 plan-to-plan bound of tests/test_gpu_ncsnpp.py), the golden samples within TOL; with the switch off
    the launch table is the one recorded before this switch existed (tests/golden/ncsnpp_plan_rows_no_up_fold.json), with it on exactly one row changes; two forwards
    give the same bytes."""
    from naturaldiffusion_amd.ncsnpp import NCSNppEngine
    from naturaldiffusion_amd._lib import lib
    dev = torch.device("cuda:0")
    fx = np.load(golden_dir / "ncsnpp_forward.npz")
    g = torch.Generator().manual_seed(40 + B)
    x = torch.randn(B, 3, 32, 32, generator=g)
    labels = torch.rand(B, generator=g) * 999
    x[:2] = torch.from_numpy(fx["x"]); labels[:2] = torch.from_numpy(fx["labels"])
    xd, ld = x.to(dev), labels.to(dev)
    try:
        assert lib.natinf_set_fuse_up_fold(0) == 0
        off = NCSNppEngine(flat, max_batch=B, device=dev)                 # the switch is read when the plan is built
        assert lib.natinf_set_fuse_up_fold(1) == 0
        on = NCSNppEngine(flat, max_batch=B, device=dev)
    finally:
        lib.natinf_set_fuse_up_fold(-1)                                   # the library's default
    rows_off, rows_on = _describe_gemms(off, B), _describe_gemms(on, B)
    assert rows_off == json.loads((golden_dir / "ncsnpp_plan_rows_no_up_fold.json").read_text())[str(B)]
    changed = [(a, b) for a, b in zip(rows_off, rows_on) if a != b]
    assert len(rows_on) == len(rows_off) and len(changed) == 1, changed
    assert changed[0][0].split()[:5] == [str(B * 1024), "256", "2304", "0", "9"] and changed[0][0].split()[6].startswith("conv_gn")
    assert changed[0][1] == f"{B * 256} 1024 1024 0 4 1 conv_gn_upfold/e2"          # the ISSUED shape: low-resolution M, four phases x 256 channels, K = 4 cin
    y_off = off(xd, ld).clone()
    y_on = on(xd, ld).clone()
    y_on2 = on(xd, ld).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(y_on).all()
    assert torch.equal(y_on, y_on2)
    ref = torch.from_numpy(fx["y"])
    e_plan, e_gold = _rel(y_on.cpu(), y_off.cpu()), _rel(y_on[:2].cpu(), ref)
    print(f"B={B}: fold on vs off {e_plan:.3e}; golden samples {e_gold:.3e} (off: {_rel(y_off[:2].cpu(), ref):.3e})")
    assert e_plan < 2e-2, e_plan
    assert e_gold <= TOL, e_gold
