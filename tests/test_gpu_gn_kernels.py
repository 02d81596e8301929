"""The GroupNorm, output-head and glue kernels of the NCSN++ / AutoencoderKL engines ALONE against fp64 (tests/gn_kernel_cases.py: cases, references, radii with their
derivations, comparators; their attainability and the mutants they catch: tests/test_gn_kernels_host.py), through the natinf_debug_gn_* / _head_conv / _time_embed /
_stem_im2col / _pack_* / _nhwc_to_nchw entry points of include/natinf_ncsnpp.h -- the launches the plans themselves make.  Every output sits between canary rows that
must come back untouched and is pre-filled with a sentinel (an element the kernel does not write fails); no case and no element is left out of a comparison.  The
worst error / radius per kernel goes to test_records/gn_kernels.json (a directory git ignores).

Worst figures measured on an MI355X (each test prints its own; 1 would be the edge of the radius or interval; for bf16 outputs the half ulp of the output's own
rounding is not counted, so 0.000 means `below the output's rounding`), the default build and the -DNATINF_LDS_POISON build alike:
  k_gn_stats 0.402 of the interval (C 384, HW 64, one_hot_group, out_mul -log2 e; 336 launches) -- the host restatement's figure to all 16 digits, as is
    k_gn_finalize's: with a fixed summation order the float32 restatement reproduces the kernel's worst element;
  k_gn_finalize 0.672 (one source, C 128, tps 1, one_hot_group: the chain is five links long, the interval at its narrowest; 144 launches, `const` -- the clamp and
    the full cancellation -- at 0.10), exact tables 0.016 of 1e-5 max |table|;
    k_gn_stats inside k_gn_finalize's interval of the same x at 0.561, k_gn_finalize inside k_gn_stats' at 0.138;
  k_gn_fold 0.500 of fold u sum |p| (fold 2: one addition, half an ulp), the quarter-integer family equal to fp64 in all 12 cases;
  k_gn_apply 0.379 (C 384, side 32, SiLU, pad 1, ld 448), borders zero bits, xr the bytes / inside 3u mean|x|, no canary row touched in 20 cases;
  k_head_conv: the exact family equal to fp64 bit for bit at ld 128 and 192, the one-hot family below the output's rounding in all 18 launches, the engine-fed random
    family 0.151 of its (wide) radius with its tables at 0.052 of their interval;
  k_time_embed below the output's rounding on the six sampler labels, 0.273 over 8,200 labels (B = 8200: every row written), sin^2 + cos^2 at 0.997 of its bound;
    k_stem_im2col, the four k_pack_conv forms, k_pack_transpose, k_nhwc_to_nchw_f32: the bytes.
All 67 tests pass and no kernel was changed.  One defect was found by reading, in a launch: the plan launched k_time_embed (one thread per element, no grid stride)
under grid1d's default cap of 4096 blocks, so a forward at B >= 8193 left the embeddings of samples 8192 .. unwritten without an error; the plan and the entry point
now pass the uncapped grid (test_time_embed_beyond_8192_samples).  The other preconditions the kernels leave to their launchers (include/natinf_ncsnpp.h, DESIGN.md
section 4) are refused by the entry points, and no plan builder of the library reaches outside them."""
import json
import os

import numpy as np
import pytest
import torch

import gn_kernel_cases as K

pytestmark = pytest.mark.gpu

WORST = {}
NAN = float("nan")


def _dev(a):
    a = np.array(a, order="C")                                          # a copy: the cases are shared and read-only
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype)
    return torch.from_numpy(a.view(view)).cuda()


def _record(repo_root, kernel, case, ratio):
    w = WORST.setdefault(kernel, {"worst_error_over_radius": 0.0, "case": None, "cases": 0})
    w["cases"] += 1
    if w["case"] is None or ratio > w["worst_error_over_radius"]:
        w["worst_error_over_radius"], w["case"] = float(ratio), case
    os.makedirs(repo_root / "test_records", exist_ok=True)
    (repo_root / "test_records" / "gn_kernels.json").write_text(json.dumps(WORST, indent=1))


class Out:
    """[pad + rows + pad][ld] of a sentinel (bf16: 0x7b7b, fp32: NaN); the kernel gets the middle rows"""

    def __init__(self, rows, ld, f32=False, pad=2):
        self.rows, self.ld, self.pad, self.f32 = rows, ld, pad, f32
        self.t = torch.full((rows + 2 * pad, ld), NAN if f32 else K.SENTINEL, dtype=torch.float32 if f32 else torch.int16, device="cuda")

    @property
    def ptr(self):
        return int(self.t.data_ptr()) + self.pad * self.ld * (4 if self.f32 else 2)

    def host(self):
        """the middle rows, after checking the canaries"""
        h = self.t.cpu().numpy()
        h = h if self.f32 else h.view(np.uint16)
        edge = np.concatenate([h[:self.pad], h[-self.pad:]])
        assert np.isnan(edge).all() if self.f32 else (edge == K.SENTINEL).all(), "a canary row around the output was written"
        return h[self.pad:-self.pad]


def _api():
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    return lib, check, ptr, stream_ptr


def _gn_stats(xbits, ld, C, HW, Bn, gamma, beta, out_mul):
    lib, check, ptr, stream_ptr = _api()
    xd, gd, bd = _dev(xbits), _dev(gamma), _dev(beta)
    sc, sh = Out(Bn, C, f32=True), Out(Bn, C, f32=True)
    check(lib.natinf_debug_gn_stats(ptr(xd), ld, C, HW, Bn, ptr(gd), ptr(bd), sc.ptr, sh.ptr, 1e-6, out_mul, stream_ptr()), "natinf_debug_gn_stats")
    torch.cuda.synchronize()
    return sc, sh


def _gn_finalize(c, out_mul):
    lib, check, ptr, stream_ptr = _api()
    q0, q1, t0, t1, HW = c["case"]
    p0, p1 = _dev(c["P0"]), (_dev(c["P1"]) if q1 else None)
    gd, bd = _dev(c["gamma"]), _dev(c["beta"])
    sc, sh = Out(K.B, c["C"], f32=True), Out(K.B, c["C"], f32=True)
    check(lib.natinf_debug_gn_finalize(ptr(p0), t0, q0, ptr(p1) or None, t1, q1, c["C"], HW, K.B, ptr(gd), ptr(bd), sc.ptr, sh.ptr, 1e-6, out_mul, stream_ptr()),
          "natinf_debug_gn_finalize")
    torch.cuda.synchronize()
    return sc.host(), sh.host()


@pytest.mark.parametrize("C,HW", K.STATS_SHAPES)
def test_gn_stats(C, HW, repo_root):
    """k_gn_stats: every table element inside its interval, every input family, ld = C and C + 64 (the other channels hold 1e4), out_mul 1 and -log2 e"""
    failures = []
    for fam in K.STATS_FAMILIES:
        c = K.stats_input(C, HW, fam)
        for ld in (C, C + 64):
            xbits = K.in_ld(K.bits_of(c["x"]), ld)
            for om in K.OUT_MULS:
                sc, sh = _gn_stats(xbits, ld, C, HW, K.B, c["gamma"], c["beta"], om)
                bad, ratio = K.check_table(K.stats_interval(C, HW, fam, om), sc.host(), sh.host())
                print(f"\ngn_stats {c['name']} ld {ld} out_mul {om:.3f}: {bad} elements outside, worst error / radius = {ratio:.3f}")
                _record(repo_root, "k_gn_stats", f"{c['name']}-ld{ld}-mul{om:.3f}", ratio)
                if bad:
                    failures.append((c["name"], ld, om, bad, ratio))
    assert not failures, failures


@pytest.mark.parametrize("case", K.FIN_CASES, ids=lambda v: "q%d+%d-tps%d.%d-HW%d" % v)
def test_gn_finalize(case, repo_root):
    """k_gn_finalize: one and two sources, every tps; random tables inside the interval, exact tables within 1e-5 of max |table|"""
    failures = []
    for fam in K.FIN_FAMILIES:
        c = K.fin_case(case, fam)
        for om in K.OUT_MULS:
            sc, sh = _gn_finalize(c, om)
            iv = K.fin_interval(c, om)
            bad, ratio = K.check_table_exact(iv, sc, sh) if fam == "exact" else K.check_table(iv, sc, sh)
            print(f"\ngn_finalize {c['name']} out_mul {om:.3f}: {bad} elements outside, worst error / radius = {ratio:.4f}")
            _record(repo_root, "k_gn_finalize (exact tables, / 1e-5 max|table|)" if fam == "exact" else "k_gn_finalize", f"{c['name']}-mul{om:.3f}", ratio)
            if bad:
                failures.append((c["name"], om, bad, ratio))
    assert not failures, failures


@pytest.mark.parametrize("C,HW,tps", [(128, 64, 2), (256, 256, 8), (384, 64, 4), (512, 16, 1)])
def test_stats_and_finalize_agree(C, HW, tps, repo_root):
    """k_gn_stats on x and k_gn_finalize on the fp64-summed quad partials of the same x: each table inside the other kernel's interval"""
    c = K.stats_input(C, HW, "randn")
    fc, iv_f = K.fin_from_x(c, tps)
    for om in K.OUT_MULS:
        sc, sh = _gn_stats(K.bits_of(c["x"]), C, C, HW, K.B, c["gamma"], c["beta"], om)
        fsc, fsh = _gn_finalize(fc, om)
        bad_sf, r_sf = K.check_table(iv_f(om), sc.host(), sh.host())
        bad_fs, r_fs = K.check_table(K.stats_interval(C, HW, "randn", om), fsc, fsh)
        print(f"\nC{C} HW{HW} tps{tps} out_mul {om:.3f}: stats in finalize's interval {r_sf:.3f}, finalize in stats' interval {r_fs:.3f}")
        _record(repo_root, "k_gn_stats inside k_gn_finalize's interval", f"C{C}-HW{HW}-tps{tps}-mul{om:.3f}", r_sf)
        _record(repo_root, "k_gn_finalize inside k_gn_stats' interval", f"C{C}-HW{HW}-tps{tps}-mul{om:.3f}", r_fs)
        assert bad_sf == 0 and bad_fs == 0


@pytest.mark.parametrize("quads", K.FOLD_QUADS)
def test_gn_fold(quads, repo_root):
    """k_gn_fold: the exact family bit for bit, the random one within fold u sum |p|; sample 1 is 100 x larger"""
    lib, check, ptr, stream_ptr = _api()
    failures = []
    for tps, fold in K.FOLD_SHAPES:
        for exact in (True, False):
            c = K.fold_case(quads, tps, fold, exact)
            pd = _dev(c["P"])
            out = Out(K.FOLD_B * (tps // fold), 2 * quads, f32=True)
            check(lib.natinf_debug_gn_fold(ptr(pd), tps, quads, fold, K.FOLD_B, out.ptr, stream_ptr()), "natinf_debug_gn_fold")
            torch.cuda.synchronize()
            bad, ratio = K.check_fold(c, out.host().reshape(K.FOLD_B, tps // fold, quads, 2))
            print(f"\ngn_fold {c['name']}: {bad} elements outside, worst error / radius = {ratio:.3f}")
            _record(repo_root, "k_gn_fold", c["name"], ratio)
            if bad:
                failures.append((c["name"], bad, ratio))
    assert not failures, failures


@pytest.mark.parametrize("case", K.APPLY_CASES, ids=lambda v: "C%d-side%d-mode%d-pad%d-act%d-xr%d-ld%d" % v)
def test_gn_apply(case, repo_root):
    """k_gn_apply: every element of the (padded) output inside [rne(y - delta), rne(y + delta)], the border zero bits, xr the bytes of x (none / up) or the mean of
    the four raw values (down).  The sentinel shows an unwritten element of any sample's ragged last row block; the canary rows (8 pixels on each side of y and of
    xr) show a write beyond the LAST sample's -- an overrun of sample b into the first rows of sample b + 1 is overwritten by that sample's own values and is not seen"""
    lib, check, ptr, stream_ptr = _api()
    C, side, mode, pad, act, xr, ld = case
    c = K.apply_case(case)
    d, dp, _, _ = K.apply_geometry(case)
    logW = side.bit_length() - 1
    xd, sd, hd = _dev(c["xbits"]), _dev(c["scale"]), _dev(c["shift"])
    y = Out(K.B * dp * dp, C, pad=8)
    xo = Out(K.B * d * d, C, pad=8) if xr else None
    check(lib.natinf_debug_gn_apply(ptr(xd), ld, C, logW, 2 * logW, K.B, ptr(sd), ptr(hd), y.ptr, xo.ptr if xr else None, act, mode, pad, stream_ptr()),
          "natinf_debug_gn_apply")
    torch.cuda.synchronize()
    bad, ratio = K.check_apply(c, y.host().reshape(K.B, dp, dp, C), xo.host().reshape(K.B, d, d, C) if xr else None)
    print(f"\ngn_apply {c['name']}: {bad} elements outside, worst (|k - y| - half ulp) / delta = {ratio:.3f}")
    _record(repo_root, "k_gn_apply", c["name"], ratio)
    assert bad == 0


def _head(xbits, ld, sc_ptr, sh_ptr, w16_ptr, bias):
    lib, check, ptr, stream_ptr = _api()
    xd, bd = _dev(K.in_ld(xbits, ld)), _dev(bias)
    out = Out(K.HEAD_B * 3 * 32, 32, f32=True, pad=4)
    check(lib.natinf_debug_head_conv(ptr(xd), ld, K.HEAD_B, sc_ptr, sh_ptr, w16_ptr, ptr(bd), out.ptr, stream_ptr()), "natinf_debug_head_conv")
    torch.cuda.synchronize()
    return out.host().reshape(K.HEAD_B, 3, 32, 32)


@pytest.mark.parametrize("ld", K.HEAD_LDS)
def test_head_conv_exact(ld, repo_root):
    """k_head_conv, the exact family: integers times halves, the activation is t itself: the output equals fp64 bit for bit -- a wrong tap, channel half, pixel, or a
    border that holds g(shift) = -40 changes an integer.  Rows 3 .. 15 of the weight buffer hold 1e4 and must not reach the output."""
    from naturaldiffusion_amd._lib import ptr
    e = K.head_exact_case()
    sd, hd, wd = _dev(e["scale"]), _dev(e["shift"]), _dev(e["w16"])
    out = _head(e["xbits"], ld, ptr(sd), ptr(hd), ptr(wd), e["bias"])
    diff = int((~(out.astype(np.float64) == e["y"])).sum())
    _record(repo_root, "k_head_conv (exact family: elements that differ)", f"ld{ld}", float(diff))
    assert diff == 0


@pytest.mark.parametrize("ld", K.HEAD_LDS)
def test_head_conv_onehot(ld, repo_root):
    """k_head_conv with one weight 1.0: the output is the kernel's own bf16 activation of one shifted pixel, inside [rne(g - dg), rne(g + dg)], t over [-100, 100]"""
    from naturaldiffusion_amd._lib import ptr
    o = K.head_onehot_case()
    sd, hd = _dev(o["scale"]), _dev(o["shift"])
    failures = []
    for hot in K.ONE_HOT:
        wd = _dev(K.head_pack(K.onehot_weights(*hot)))
        bad, ratio = K.check_head_onehot(o, hot, _head(o["xbits"], ld, ptr(sd), ptr(hd), ptr(wd), np.zeros(3, np.float32)))
        print(f"\nhead one-hot (channel, tap, output) {hot} ld {ld}: {bad} elements outside, worst (|k - g| - half ulp) / dg = {ratio:.3f}")
        _record(repo_root, "k_head_conv (one-hot)", f"{hot}-ld{ld}", ratio)
        if bad:
            failures.append((hot, bad, ratio))
    assert not failures, failures


@pytest.mark.parametrize("ld", K.HEAD_LDS)
def test_head_conv_random(ld, repo_root):
    """k_head_conv as the engine feeds it: tables from k_gn_stats (out_mul = -log2 e), weights from k_pack_conv (chunked, wmul = -ln 2) into a buffer whose rows 3 .. 15
    hold 1e4, against the fp64 convolution of SiLU(GroupNorm(x)) with the unrounded weights.  The radius is a bound, wide by construction: the indexing rests on the
    exact and one-hot families."""
    lib, check, ptr, stream_ptr = _api()
    r = K.head_random_input()
    y, rad, iv = K.head_random_reference()
    sc, sh = _gn_stats(K.in_ld(r["xbits"], ld), ld, K.HEAD_C, 1024, K.HEAD_B, r["gamma"], r["beta"], K.NEG_LOG2E)
    bad_t, ratio_t = K.check_table(iv, sc.host(), sh.host())
    wsrc = _dev(r["w"])
    w16 = Out(16, K.HEAD_K)
    w16.t[w16.pad:-w16.pad] = int(K.head_pack(np.zeros((3, K.HEAD_C, 9)))[3, 0])              # bf16(1e4) everywhere; the pack then writes rows 0 .. 2
    check(lib.natinf_debug_pack_conv(ptr(wsrc), w16.ptr, 3, K.HEAD_C, 9, K.HEAD_K, 0, K.HEAD_C, 1, float(K.NEG_LN2_F), stream_ptr()), "natinf_debug_pack_conv")
    out = _head(r["xbits"], ld, sc.ptr, sh.ptr, w16.ptr, r["bias"])
    bad, ratio = K.check_head_random(y, rad, out)
    print(f"\nhead random ld {ld}: {bad} elements outside, worst error / radius = {ratio:.3f} (tables: {ratio_t:.3f})")
    _record(repo_root, "k_head_conv (random, engine-fed)", f"ld{ld}", ratio)
    assert bad == 0 and bad_t == 0


def test_time_embed(repo_root):
    """k_time_embed: the sampler's labels (node x 999) inside [rne(y - delta), rne(y + delta)]; columns j and j + 64 satisfy sin^2 + cos^2 = 1 to bf16 accuracy"""
    lib, check, ptr, stream_ptr = _api()
    ld = _dev(K.LABELS)
    out = Out(len(K.LABELS), 128)
    check(lib.natinf_debug_time_embed(ptr(ld), out.ptr, len(K.LABELS), stream_ptr()), "natinf_debug_time_embed")
    torch.cuda.synchronize()
    bad, ratio, pyth = K.check_embed(out.host())
    print(f"\ntime_embed: {bad} elements outside, worst (|k - y| - half ulp) / delta = {ratio:.3f}, |sin^2 + cos^2 - 1| / bound = {pyth:.3f}")
    _record(repo_root, "k_time_embed", "labels", ratio)
    assert bad == 0


def test_time_embed_beyond_8192_samples(repo_root):
    """k_time_embed has one thread per element and no grid stride: at B = 8200 (4100 blocks) every row must be written.  The plan used to launch it under a cap of
    4096 blocks, which left the rows of samples 8192 .. unwritten; the sentinel shows such a row."""
    lib, check, ptr, stream_ptr = _api()
    labels = (np.arange(K.BIG_BATCH, dtype=np.float64) * (999.0 / (K.BIG_BATCH - 1))).astype(np.float32)
    ld = _dev(labels)
    out = Out(K.BIG_BATCH, 128)
    check(lib.natinf_debug_time_embed(ptr(ld), out.ptr, K.BIG_BATCH, stream_ptr()), "natinf_debug_time_embed")
    torch.cuda.synchronize()
    h = out.host()
    assert not (h[8192:] == K.SENTINEL).any(), "rows of samples 8192 .. were not written"
    bad, ratio, pyth = K.check_embed(h, labels)
    print(f"\ntime_embed B {K.BIG_BATCH}: {bad} elements outside, worst (|k - y| - half ulp) / delta = {ratio:.3f}, |sin^2 + cos^2 - 1| / bound = {pyth:.3f}")
    _record(repo_root, "k_time_embed", f"B{K.BIG_BATCH}", ratio)
    assert bad == 0


def test_stem_im2col(repo_root):
    """k_stem_im2col: the bytes of the numpy gather, columns 27 .. 63 zero bits, all four image edges"""
    lib, check, ptr, stream_ptr = _api()
    c = K.stem_case()
    xd = _dev(c["x"])
    out = Out(K.STEM_B * 1024, 64, pad=4)
    check(lib.natinf_debug_stem_im2col(ptr(xd), out.ptr, K.STEM_B, stream_ptr()), "natinf_debug_stem_im2col")
    torch.cuda.synchronize()
    diff = int((out.host() != c["y"]).sum())
    _record(repo_root, "k_stem_im2col (elements that differ)", "B2", float(diff))
    assert diff == 0


@pytest.mark.parametrize("form", K.PACK_FORMS, ids=lambda v: "N%d-Cin%d-taps%d-ld%d-koff%d-ts%d-chunked%d-mul%.3f" % v)
def test_pack_conv(form, repo_root):
    """k_pack_conv: exactly the addressed elements of a sentinel-filled destination change, each to bf16(float32(src) float32(wmul))"""
    lib, check, ptr, stream_ptr = _api()
    N, Cin, taps, dst_ld, koff, ts, chunked, wmul = form
    c = K.pack_form_case(form)
    sd = _dev(c["src"])
    out = Out(N, dst_ld)
    check(lib.natinf_debug_pack_conv(ptr(sd), out.ptr, N, Cin, taps, dst_ld, koff, ts, chunked, wmul, stream_ptr()), "natinf_debug_pack_conv")
    torch.cuda.synchronize()
    diff = int((out.host() != c["y"]).sum())
    _record(repo_root, "k_pack_conv (elements that differ)", "N%d-Cin%d-taps%d" % form[:3], float(diff))
    assert diff == 0


def test_pack_transpose_and_nhwc_to_nchw(repo_root):
    """k_pack_transpose (K != N, ld > K) and k_nhwc_to_nchw_f32 (ld > C; the exact widening of every bf16 value, sub-normals included): the bytes"""
    lib, check, ptr, stream_ptr = _api()
    Kd, N, ld = K.TRANSPOSE_CASE
    c = K.transpose_case()
    sd = _dev(c["src"])
    out = Out(N, ld)
    check(lib.natinf_debug_pack_transpose(ptr(sd), out.ptr, Kd, N, ld, stream_ptr()), "natinf_debug_pack_transpose")
    torch.cuda.synchronize()
    d1 = int((out.host() != c["y"]).sum())
    Bn, HW, C, xld = K.NCHW_CASE
    c = K.nchw_case()
    xd = _dev(c["x"])
    o2 = Out(Bn * C, HW, f32=True)
    check(lib.natinf_debug_nhwc_to_nchw(ptr(xd), xld, C, HW, Bn, o2.ptr, stream_ptr()), "natinf_debug_nhwc_to_nchw")
    torch.cuda.synchronize()
    d2 = int((o2.host().view(np.uint32).reshape(Bn, C, HW) != c["y"]).sum())
    _record(repo_root, "k_pack_transpose (elements that differ)", "K%d-N%d-ld%d" % K.TRANSPOSE_CASE, float(d1))
    _record(repo_root, "k_nhwc_to_nchw_f32 (elements that differ)", "B%d-HW%d-C%d-ld%d" % K.NCHW_CASE, float(d2))
    assert d1 == 0 and d2 == 0
