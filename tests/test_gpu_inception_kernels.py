"""The Inception engine's stem, pool, global-average, BatchNorm-fold and im2col kernels ALONE against fp64 (tests/inception_kernel_cases.py: cases, references, radii,
comparators; their attainability and the mutants they catch: tests/test_inception_kernels_host.py), through the natinf_debug_inc_* entry points of
include/natinf_inception.h -- the launches the plan itself makes.  Every output sits between canaries that must come back untouched, is pre-filled with a sentinel
(an element the kernel does not write fails), and no case and no element is left out of a comparison.  The worst error / radius per kernel goes to
test_records/inception_kernels.json (a directory git ignores).

Worst figures measured on an MI355X (each test prints its own; 1 would be the edge of the radius; the part of an error inside the output format's own rounding,
half a 16-bit ulp, is not counted, so 0.000 means `below the output's rounding`):
  k_inc_stem 0.487 ((640, 16), half; bf16 0.427), 0.000 at (299, 299) and (1, 1); the eight k_inc_pool instances 0.000, every maximum equal;
  k_inc_global_avg 0.019 (HW 64, half); k_inc_pack |hi + lo - W'| at 0.984 of (2^-17 + 3u) |W'|, hi and bias inside; k_inc_pack_f16 0.594, every scale equal;
  k_inc_im2col the same bytes.
All 80 tests pass: no defect found, no kernel changed."""
import json
import os

import numpy as np
import pytest
import torch

import inception_kernel_cases as K

pytestmark = pytest.mark.gpu

SENTINEL = 0x7b7b                                                       # a finite 16-bit pattern in both formats that no case produces
WORST = {}


def _dev(a):
    a = np.array(a, order="C")                                          # a copy: the cases are shared and read-only
    view = {np.dtype(np.uint16): np.int16}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(view)).cuda()


def _host16(t):
    return t.cpu().numpy().view(np.uint16)


def _record(repo_root, kernel, case, ratio):
    w = WORST.setdefault(kernel, {"worst_error_over_radius": 0.0, "case": None, "cases": 0})
    w["cases"] += 1
    if w["case"] is None or ratio > w["worst_error_over_radius"]:
        w["worst_error_over_radius"], w["case"] = float(ratio), case
    os.makedirs(repo_root / "test_records", exist_ok=True)
    (repo_root / "test_records" / "inception_kernels.json").write_text(json.dumps(WORST, indent=1))


def _padded(rows, ld, value=SENTINEL, pad=1):
    """a [pad + rows + pad][ld] int16 buffer full of `value`: the kernel gets the middle rows"""
    return torch.full((rows + 2 * pad, ld), value, dtype=torch.int16, device="cuda")


def _canaries_ok(buf, pad=1):
    h = _host16(buf)
    return bool(np.all(h[:pad] == SENTINEL) and np.all(h[-pad:] == SENTINEL))


@pytest.mark.parametrize("row_width", [64, 32])
@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("H,W", K.STEM_SIZES, ids=lambda v: str(v))
def test_stem(H, W, f16, row_width, repo_root):
    """k_inc_stem: every element of the 2 x 149 x 149 patch rows within [rne16(y - delta), rne16(y + delta)], the pad columns zero bits, the 299 x 299 input equal to
    rne16(2 x - 1); the fp32 input holding the uint8 input's values gives the same bytes"""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    c = K.stem_case(H, W)
    rows = K.STEM_B * 149 * 149
    got = {}
    for kind, img in ((0, c["u8"]), (1, c["f32"])):
        d = _dev(img)
        out = _padded(rows, row_width)
        check(lib.natinf_debug_inc_stem(ptr(d), kind, K.STEM_B, H, W, f16, row_width, ptr(out) + 2 * row_width, stream_ptr()), "natinf_debug_inc_stem")
        torch.cuda.synchronize()
        assert _canaries_ok(out), "a canary row around the patch rows was written"
        got[kind] = _host16(out)[1:-1]
    bad, ratio = K.check_stem(c, got[0], f16)
    print(f"\nstem {c['name']} {'f16' if f16 else 'bf16'} rows of {row_width}: {bad} elements outside, worst (|k - y| - half ulp) / delta = {ratio:.3f}")
    _record(repo_root, "k_inc_stem", f"{c['name']}-{'f16' if f16 else 'bf16'}-{row_width}", ratio)
    assert bad == 0
    assert np.array_equal(got[0], got[1]), "the fp32 input gives other bytes than the uint8 input"


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("geom", K.POOL_GEOMS, ids=lambda g: "s%dp%d-%dx%d-B%d-C%d-ld%d" % g)
def test_pool(geom, f16, repo_root):
    """k_inc_pool<f16, mode, stride>: the maximum as a value, the average within 10u sum|x| / count (exactly 0.5 on the constant input), every input family, into a
    channel slice of a wider buffer whose other channels must survive"""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    stride, pad, H, W, B, C, x_ld = geom
    out_ld = C + 8
    failures = []
    for g, fam in K.pool_cases():
        if g != geom:
            continue
        c = K.pool_case(geom, fam, f16)
        xd = _dev(c["x"])
        rows = B * c["Ho"] * c["Wo"]
        for mode in (0, 1):
            out = _padded(rows, out_ld)
            check(lib.natinf_debug_inc_pool(f16, mode, stride, pad, B, H, W, C, ptr(xd), x_ld, ptr(out) + 2 * out_ld, out_ld, stream_ptr()), "natinf_debug_inc_pool")
            torch.cuda.synchronize()
            h = _host16(out)
            assert _canaries_ok(out) and np.all(h[1:-1, C:] == SENTINEL), "the pool wrote outside its channel slice"
            bad, ratio = K.check_pool(c, mode, h[1:-1, :C])
            print(f"\npool {c['name']} {'avg' if mode else 'max'}: {bad} elements outside, worst (|k - y| - half ulp) / delta = {ratio:.3f}")
            _record(repo_root, f"k_inc_pool<{f16},{mode},{stride}>", c["name"], ratio)
            if bad:
                failures.append((c["name"], "avg" if mode else "max", bad))
    assert not failures, failures


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,HW,C", K.GAVG_CASES)
def test_global_average(B, HW, C, f16, repo_root):
    """k_inc_global_avg: the fp32 output within HW u mean|x| of the fp64 mean"""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    c = K.gavg_case(B, HW, C, f16)
    xd = _dev(c["x"])
    out = torch.full((B + 2, C), float("nan"), dtype=torch.float32, device="cuda")
    check(lib.natinf_debug_inc_global_avg(f16, B, HW, C, ptr(xd), ptr(out) + 4 * C, stream_ptr()), "natinf_debug_inc_global_avg")
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert np.isnan(h[0]).all() and np.isnan(h[-1]).all(), "a canary row around the means was written"
    bad, ratio = K.check_gavg(c, h[1:-1])
    print(f"\nglobal average {c['name']}: {bad} elements outside, worst |out - y| / delta = {ratio:.3f}")
    _record(repo_root, "k_inc_global_avg", c["name"], ratio)
    assert bad == 0


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("geom", K.PACK_GEOMS, ids=lambda g: "N%d-Np%d-C%d-Cp%d-%dx%d-Kp%d" % g)
def test_pack(geom, f16, repo_root):
    """k_inc_pack / k_inc_pack_f16: the folded filters (two bf16 terms, or one half term and the row's power-of-two scale), the bias, the zeros of every pad"""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    N, Np, C, Cp, kh, kw, Kp = geom
    c = K.pack_case(geom)
    d = {n: _dev(c[n]) for n in ("w", "gamma", "beta", "mean", "var")}
    ld = Kp if f16 else 2 * Kp
    wp = _padded(Np, ld)
    bias = torch.full((Np + 2,), float("nan"), dtype=torch.float32, device="cuda")
    deq = torch.full((Np + 2,), float("nan"), dtype=torch.float32, device="cuda")
    check(lib.natinf_debug_inc_pack(f16, ptr(d["w"]), ptr(d["gamma"]), ptr(d["beta"]), ptr(d["mean"]), ptr(d["var"]), N, Np, C, Cp, kh, kw, Kp, ptr(wp) + 2 * ld,
                                    ptr(bias) + 4, (ptr(deq) + 4) if f16 else None, stream_ptr()), "natinf_debug_inc_pack")
    torch.cuda.synchronize()
    bh, dh = bias.cpu().numpy(), deq.cpu().numpy()
    assert _canaries_ok(wp) and np.isnan(bh[0]) and np.isnan(bh[-1]) and np.isnan(dh[0]) and np.isnan(dh[-1]), "a canary was written"
    assert f16 or np.isnan(dh).all(), "the bf16 pack wrote deq"
    fails, ratio = K.check_pack(c, f16, _host16(wp)[1:-1], bh[1:-1], dh[1:-1] if f16 else None)
    print(f"\npack {c['name']} {'half' if f16 else 'bf16'}: failures {fails}, worst figure = {ratio:.3f}")
    _record(repo_root, "k_inc_pack_f16" if f16 else "k_inc_pack", c["name"], ratio)
    assert not any(fails.values()), fails


@pytest.mark.parametrize("case", K.IM2COL_CASES, ids=lambda v: "B%d-%dx%d-ld%d-C%d-%dx%d-s%d-p%d.%d-Kp%d" % v)
def test_im2col(case, repo_root):
    """k_inc_im2col: the bytes of the numpy gather"""
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    B, H, W, ld, C, kh, kw, stride, ph, pw, Kp = case
    c = K.im2col_case(case)
    xd = _dev(c["x"])
    rows = c["y"].shape[0]
    out = _padded(rows, Kp)
    check(lib.natinf_debug_inc_im2col(B, H, W, ld, C, kh, kw, stride, ph, pw, Kp, ptr(xd), ptr(out) + 2 * Kp, stream_ptr()), "natinf_debug_inc_im2col")
    torch.cuda.synchronize()
    assert _canaries_ok(out), "a canary row around the im2col matrix was written"
    diff = int((_host16(out)[1:-1] != c["y"]).sum())
    _record(repo_root, "k_inc_im2col", "B%d-%dx%d-C%d-%dx%d" % (B, H, W, C, kh, kw), float(diff))
    assert diff == 0
