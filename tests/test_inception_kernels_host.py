"""The references and comparators of tests/inception_kernel_cases.py, shown sound on the CPU before a GPU is involved: the numpy fp64 references equal torch's own
fp64 operators (an anchor independent of the restated oracle), a numpy-float32 restatement of every kernel in its own operation order passes every case that
tests/test_gpu_inception_kernels.py runs, and each mutant -- the slips a tolerance of 3e-2 of the feature maximum lets through -- fails a case named here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import inception_kernel_cases as K


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) <= tol * max(1.0, float(np.max(np.abs(b))))


def test_half_format_helpers():
    v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11 + 2.0 ** -30), 2.0 ** -25, 2.0 ** -25 * 1.01, 65519.9, 65520.0, 0.1])
    assert K.rne_f16(v).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -10), 0.0, 2.0 ** -24, 65504.0, np.inf, float(np.float16(0.1))]
    assert K.half_ulp_f16(np.array([1.0, 1.99, 2.0, 2.0 ** -14, 2.0 ** -20, 0.0])).tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25]
    r = (np.random.default_rng(0).standard_normal(4096) * 7).astype(np.float32)
    assert np.array_equal(K.f16_bits_to_f64(K.f32_to_f16_bits(r)), K.rne_f16(r.astype(np.float64)))
    assert K.f16_bits_to_f64(K.f32_to_f16_bits(np.float32([1e6, -1e6]))).tolist() == [65504.0, -65504.0]            # inc_cvt16 saturates
    assert K._pow2_above(np.array([0.0, 0.5, 0.75, 1.0, 3.0, 0.1])).tolist() == [1.0, 1.0, 1.0, 2.0, 4.0, 0.125]


# ---- the fp64 references against torch's own fp64 operators ------------------------------------------------------------------------------------------------------

def test_references_equal_torch_fp64():
    for H, W in K.STEM_SIZES[:6]:
        c = K.stem_case(H, W)
        v = torch.from_numpy(c["f32"].astype(np.float64))
        r = 2.0 * TF.interpolate(v, size=(299, 299), mode="bilinear", align_corners=False) - 1.0
        cols = TF.unfold(r, 3, stride=2)                                     # [B][c 9 + tap][149 149]
        want = cols.reshape(K.STEM_B, 3, 9, 149 * 149).permute(0, 3, 2, 1).reshape(-1, 27).numpy()
        assert _close(c["y"], want), (H, W)
    for geom in K.POOL_GEOMS:
        stride, pad = geom[:2]
        for fam in ("normal", "all_negative"):
            c = K.pool_case(geom, fam, 1)
            x = torch.from_numpy(np.array(c["xv"])).permute(0, 3, 1, 2)
            assert np.array_equal(c["max"], TF.max_pool2d(x, 3, stride, pad).permute(0, 2, 3, 1).numpy()), c["name"]
            assert _close(c["avg"], TF.avg_pool2d(x, 3, stride, pad, count_include_pad=False).permute(0, 2, 3, 1).numpy()), c["name"]
    for B, HW, C in K.GAVG_CASES:
        c = K.gavg_case(B, HW, C, 0)
        x = torch.from_numpy(np.array(c["xv"])).permute(0, 2, 1).reshape(B, C, HW, 1)
        assert _close(c["y"], TF.adaptive_avg_pool2d(x, (1, 1)).reshape(B, C).numpy())
    for case in K.IM2COL_CASES:
        B, H, W, ld, C, kh, kw, stride, ph, pw, Kp = case
        c = K.im2col_case(case)
        x = torch.from_numpy(c["x"][..., :C].astype(np.float64)).permute(0, 3, 1, 2)
        cols = TF.unfold(x, (kh, kw), stride=stride, padding=(ph, pw))       # [B][c kh kw + tap][L]
        want = cols.reshape(B, C, kh * kw, -1).permute(0, 3, 2, 1).reshape(-1, kh * kw * C).numpy()
        assert np.array_equal(c["y"][:, :kh * kw * C].astype(np.float64), want) and not c["y"][:, kh * kw * C:].any(), case
    g = torch.Generator().manual_seed(3)
    for geom in K.PACK_GEOMS:
        N, Np, C, Cp, kh, kw, Kp = geom
        c = K.pack_case(geom)
        x = torch.randn(2, C, 9, 9, generator=g, dtype=torch.float64)
        t = lambda a: torch.from_numpy(np.array(a, np.float64))
        want = TF.batch_norm(TF.conv2d(x, t(c["w"]), padding=(kh // 2, kw // 2)), t(c["mean"]), t(c["var"]), t(c["gamma"]), t(c["beta"]), False, 0.0, K.EPS_BN)
        Wf = c["W"][:N, :kh * kw * Cp].reshape(N, kh, kw, Cp)[..., :C].transpose(0, 3, 1, 2)
        got = TF.conv2d(x, t(np.ascontiguousarray(Wf)), t(c["b"][:N]), padding=(kh // 2, kw // 2))
        assert _close(got.numpy(), want.numpy()), geom
        assert not c["W"][N:].any() and not c["b"][N:].any() and not c["W"][:, kh * kw * Cp:].any()
        assert not c["W"][:, :kh * kw * Cp].reshape(Np, kh * kw, Cp)[:, :, C:].any()


def test_cases_reach_the_paths_they_name():
    assert K.STEM_SIZES == ((32, 32), (40, 24), (5, 7), (1, 1), (2, 130), (640, 16), (300, 64), (299, 299)) and K.STEM_B == 2
    # (640, 16): staged (W <= 128), and some taps leave the four staged rows -- in float32, as the kernel decides it
    sy = np.float32(640) / np.float32(299.0)
    f = lambda y: np.maximum((np.float32(y) + np.float32(0.5)) * sy - np.float32(0.5), np.float32(0))
    oy = np.arange(149)
    r_lo = f(2 * oy).astype(np.int32)
    y1 = np.minimum(f(2 * oy + 2).astype(np.int32) + 1, 639)
    assert (y1 - r_lo > 3).all() and (np.minimum(f(2 * oy).astype(np.int32) + 1, 639) - r_lo <= 3).all()
    c = K.stem_case(32, 32)
    assert not np.array_equal(c["u8"][0], c["u8"][1]) and c["y"].shape == (2 * 149 * 149, 27) and (c["delta"] >= 8 * K.U).all()
    c = K.stem_case(299, 299)
    assert c["exact"] and _close(c["y"], K.patches(2.0 * c["f32"].astype(np.float64).transpose(0, 2, 3, 1) - 1.0), 0.0)
    geoms = {g[:4] for g in K.POOL_GEOMS}
    assert {(2, 0, 9, 9), (2, 0, 8, 11), (2, 0, 3, 3), (1, 1, 8, 8), (1, 1, 5, 7), (1, 1, 2, 2), (1, 1, 1, 1), (1, 1, 1, 6), (2, 1, 7, 6)} <= geoms
    assert (1, 1, 8, 8, 2, 192, 192) in K.POOL_GEOMS and 2 * 8 * (192 // 8) == 384
    ids = K.pool_cases()
    assert ((2, 0, 8, 11, 2, 72, 80), "outside_hot") in ids and ((2, 0, 9, 9, 2, 72, 80), "outside_hot") not in ids
    for f16 in (0, 1):
        c = K.pool_case((2, 0, 8, 11, 2, 72, 80), "outside_hot", f16)
        assert c["has_uncovered"] and (c["xv"][:, 7] > 5e4).all() and c["max"].max() < 10 and np.isnan(K.bits_to_f64(c["x"][..., 72:], f16)).all()
        c = K.pool_case((1, 1, 5, 7, 2, 72, 80), "post_relu", f16)
        assert 0.4 < (c["xv"] == 0).mean() < 0.6
        assert (K.pool_case((1, 1, 5, 7, 2, 72, 80), "all_negative", f16)["max"] < 0).all()
        assert (K.pool_case((1, 1, 1, 1, 2, 72, 80), "constant_half", f16)["avg"] == 0.5).all()
    for geom in K.PACK_GEOMS:
        c = K.pack_case(geom)
        assert c["var"].min() == np.float32(1e-4) and c["var"].max() == np.float32(10.0) and (c["gamma"] < 0).any()
        m = np.abs(c["W"]).max(axis=1) / c["deq"]
        assert ((m >= 0.5 + 8 * K.U) & (m <= 1 - 8 * K.U))[:geom[0]].all() and (c["deq"][geom[0]:] == 1).all()


# ---- the restatements pass every case ---------------------------------------------------------------------------------------------------------------------------

def test_restated_stem_passes():
    worst, raw = 0.0, 0.0
    for H, W in K.STEM_SIZES:
        c = K.stem_case(H, W)
        for f16 in (0, 1):
            for rw in (64, 32):
                bits, p = K.stem_restated(c, f16, rw)
                bad, ratio = K.check_stem(c, bits, f16)
                assert bad == 0, (c["name"], f16, rw, bad)
                worst = max(worst, ratio)
        raw = max(raw, float(np.max(np.abs(p.astype(np.float64) - c["y"]) / c["delta"])))
    print(f"\nrestated stem: worst |fp32 value - y| / delta = {raw:.3f}; worst comparator figure = {worst:.3f}")
    assert raw <= 0.51


def test_restated_pools_pass():
    worst = 0.0
    for geom, fam in K.pool_cases():
        for f16 in (0, 1):
            c = K.pool_case(geom, fam, f16)
            for mode in (0, 1):
                bad, ratio = K.check_pool(c, mode, K.pool_restated(c, mode))
                assert bad == 0, (c["name"], mode, bad)
                worst = max(worst, ratio)
    print(f"\nrestated pools: worst (|16-bit average - y| - half ulp) / delta = {worst:.3f}")


def test_restated_global_average_passes():
    worst = 0.0
    for B, HW, C in K.GAVG_CASES:
        for f16 in (0, 1):
            c = K.gavg_case(B, HW, C, f16)
            bad, ratio = K.check_gavg(c, K.gavg_restated(c))
            assert bad == 0, c["name"]
            worst = max(worst, ratio)
    print(f"\nrestated global average: worst |fp32 - y| / delta = {worst:.3f}")


def test_restated_packs_pass():
    worst = [0.0, 0.0]
    for geom in K.PACK_GEOMS:
        c = K.pack_case(geom)
        for f16 in (0, 1):
            fails, ratio = K.check_pack(c, f16, *K.pack_restated(c, f16))
            assert not any(fails.values()), (c["name"], f16, fails)
            worst[f16] = max(worst[f16], ratio)
    print(f"\nrestated packs: bf16 worst |hi + lo - W'| / ((2^-17 + 3u) |W'|) = {worst[0]:.3f}; half worst (|half - W' / deq| - half ulp) / (3u |W' / deq|) = {worst[1]:.3f}")


# ---- every mutant fails a named case ----------------------------------------------------------------------------------------------------------------------------

STEM_MUTANT_CASES = {"align_corners": (32, 32), "no_clamp_at_0": (32, 32), "k_channel_major": (5, 7), "bytes_over_256": (299, 299), "staged_row_off_by_one": (40, 24)}


@pytest.mark.parametrize("mutant", K.STEM_MUTANTS)
@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "f16"])
def test_stem_mutants_fail(mutant, f16):
    c = K.stem_case(*STEM_MUTANT_CASES[mutant])
    bad, _ = K.check_stem(c, K.stem_restated(c, f16, 32, mutant)[0], f16)
    print(f"\nstem mutant {mutant} on {c['name']}: {bad} elements outside")
    assert bad > 0
    assert K.check_stem(c, K.stem_restated(c, f16, 32)[0], f16)[0] == 0


def test_stem_pad_columns_are_checked():
    c = K.stem_case(5, 7)
    bits, _ = K.stem_restated(c, 0, 64)
    bits[1234, 27] = 0x8000                                                  # -0.0 in a pad column: not zero bits
    assert K.check_stem(c, bits, 0)[0] == 1


# mutant -> (geometry, family, mode)
POOL_MUTANT_CASES = {
    "count_include_pad": ((1, 1, 8, 8, 2, 72, 80), "constant_half", 1),
    "zero_pad_wins_max": ((1, 1, 5, 7, 2, 72, 80), "all_negative", 0),
    "stride2_keeps_wrong_column": ((2, 0, 9, 9, 2, 72, 80), "normal", 0),
    "last_column_dropped": ((2, 0, 8, 11, 2, 72, 80), "normal", 1),
}


@pytest.mark.parametrize("mutant", K.POOL_MUTANTS)
@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "f16"])
def test_pool_mutants_fail(mutant, f16):
    geom, fam, mode = POOL_MUTANT_CASES[mutant]
    c = K.pool_case(geom, fam, f16)
    bad, _ = K.check_pool(c, mode, K.pool_restated(c, mode, mutant))
    assert bad > 0
    assert K.check_pool(c, mode, K.pool_restated(c, mode))[0] == 0
    if mutant == "count_include_pad":                                        # the border outputs, and only they
        k = K.bits_to_f64(K.pool_restated(c, 1, mutant), f16).reshape(c["avg"].shape)
        assert (k[:, 1:-1, 1:-1] == 0.5).all() and (k[:, 0] != 0.5).all() and (k[:, :, -1] != 0.5).all()
    if mutant == "stride2_keeps_wrong_column":                               # the walker's mutant also shows in the average, and with padding
        for g2, mode2 in ((geom, 1), ((2, 1, 7, 6, 2, 72, 80), 0), ((2, 1, 7, 6, 2, 72, 80), 1)):
            c2 = K.pool_case(g2, "normal", f16)
            assert K.check_pool(c2, mode2, K.pool_restated(c2, mode2, mutant))[0] > 0


def test_pool_outside_cells_would_show():
    """a walker that lets the cell outside every window into the last output fails the `outside_hot` family (and no other)"""
    for f16 in (0, 1):
        c = K.pool_case((2, 0, 8, 11, 2, 72, 80), "outside_hot", f16)
        for mode in (0, 1):
            bits = K.pool_restated(c, mode).reshape(2, c["Ho"], c["Wo"], 72).copy()
            bits[:, -1] = K.f32_to_bits(np.float32([K.HOT]), f16)[0]
            assert K.check_pool(c, mode, bits.reshape(-1, 72))[0] == 2 * c["Wo"] * 72


def test_global_average_mutant_fails():
    for f16 in (0, 1):
        c = K.gavg_case(3, 64, 2048, f16)
        assert K.check_gavg(c, K.gavg_restated(c, "average_over_HW+1"))[0] > 0.9 * 3 * 2048
        c = K.gavg_case(2, 1, 8, f16)
        assert K.check_gavg(c, K.gavg_restated(c, "average_over_HW+1"))[0] == 16


# mutant -> (geometry, f16, the check that must fail)
PACK_MUTANT_CASES = {
    "eps_1e-5": ((32, 32, 3, 3, 3, 3, 32), (0, 1), ("hi", "half")),
    "ky_kx_swapped": ((64, 64, 48, 64, 5, 5, 1600), (0, 1), ("hi", "half")),
    "lo_zero": ((48, 64, 40, 64, 1, 7, 448), (0,), ("hi+lo",)),
    "bias_without_mean": ((80, 96, 64, 64, 1, 1, 64), (0, 1), ("bias", "bias")),
    "half_scale_one_power_off": ((48, 64, 40, 64, 7, 1, 448), (1,), ("deq",)),
}


@pytest.mark.parametrize("mutant", K.PACK_MUTANTS)
def test_pack_mutants_fail(mutant):
    geom, kinds, which = PACK_MUTANT_CASES[mutant]
    c = K.pack_case(geom)
    for f16, name in zip(kinds, which):
        fails, _ = K.check_pack(c, f16, *K.pack_restated(c, f16, mutant))
        assert fails[name] > 0, (mutant, f16, fails)
        assert not any(K.check_pack(c, f16, *K.pack_restated(c, f16))[0].values())
    if mutant == "eps_1e-5":                                                 # a 5e-4 relative change where the variance is ordinary, far more where the eps decides
        fails, _ = K.check_pack(c, 0, *K.pack_restated(c, 0, mutant))
        assert fails["hi+lo"] == 32 * 27 and fails["bias"] > 0


def test_im2col_reference_is_discriminating():
    case = K.IM2COL_CASES[0]                                                 # 3 x 3, non-square image: a transposed tap order cannot hide
    c = K.im2col_case(case)
    assert not np.array_equal(K.im2col_reference(c["x"], case, "tap_order_swapped"), c["y"])
    assert sorted({cs[10] - cs[5] * cs[6] * cs[4] for cs in K.IM2COL_CASES})[-1] > 0 and any(cs[3] > cs[4] for cs in K.IM2COL_CASES)
