"""The references and comparators of tests/gn_kernel_cases.py, shown sound on the CPU before a GPU is involved: the numpy fp64 references equal torch's own fp64
operators, every case reaches the path it is named for (asserted from the kernels' index arithmetic), a numpy-float32 restatement of every kernel in its own
summation order passes every comparator that tests/test_gpu_gn_kernels.py applies (the worst error / radius is printed), each named mutant fails on the family named
for it, and the exact families are exact."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import gn_kernel_cases as K
from row_kernel_cases import bf16_bits_to_f64, f32_to_bf16_bits

F = np.float32


def _close(a, b, tol=1e-11):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) <= tol * max(1.0, float(np.max(np.abs(b))))


def _t(a):
    return torch.from_numpy(np.array(a, np.float64))


# ---- 1. the fp64 references against torch's own fp64 operators ---------------------------------------------------------------------------------------------------

def test_references_equal_torch_fp64():
    for C, HW, fam in ((128, 64, "randn"), (384, 16, "mix"), (512, 256, "mean8"), (256, 16, "one_hot_group")):
        c = K.stats_input(C, HW, fam)
        iv = K.stats_interval(C, HW, fam, 1.0)
        want = TF.group_norm(_t(c["x"]).permute(0, 2, 1), 32, _t(c["gamma"]), _t(c["beta"]), K.EPS).permute(0, 2, 1).numpy()
        assert _close(c["x"] * iv["scale"][2][:, None, :] + iv["shift"][2][:, None, :], want, 1e-9), c["name"]
        iv2 = K.stats_interval(C, HW, fam, K.NEG_LOG2E)
        assert _close(iv2["scale"][2], iv["scale"][2] * K.NEG_LOG2E) and _close(iv2["shift"][2], iv["shift"][2] * K.NEG_LOG2E)
    for case in K.APPLY_CASES:
        C, side, mode, pad, act, xr, ld = case
        c = K.apply_case(case)
        d = K.apply_geometry(case)[0]
        v = _t(c["x"]) * _t(c["scale"])[:, None, None, :] + _t(c["shift"])[:, None, None, :]
        y = (TF.silu(v) if act else v).permute(0, 3, 1, 2)
        if mode == K.RS_UP: y = TF.interpolate(y, scale_factor=2, mode="nearest")
        elif mode == K.RS_DOWN: y = TF.avg_pool2d(y, 2)
        want = TF.pad(y, (pad, pad, pad, pad)).permute(0, 2, 3, 1).numpy()
        assert _close(c["Y"], want, 1e-12) and np.abs(want).max() < 81, c["name"]
        if mode == K.RS_DOWN:
            assert _close(c["xr_y"], TF.avg_pool2d(_t(c["x"]).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy())
        elif mode == K.RS_UP:
            up = TF.interpolate(_t(c["x"]).permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1).numpy()
            assert np.array_equal(bf16_bits_to_f64(c["xr_bits"]), up)
    e = K.head_exact_case()
    w4 = lambda w: _t(w).reshape(3, K.HEAD_C, 3, 3)
    assert np.array_equal(e["y"], TF.conv2d(_t(e["t"]).permute(0, 3, 1, 2), w4(e["w"]), _t(e["bias"]), padding=1).numpy())
    r = K.head_random_input()
    y, rad, _ = K.head_random_reference()
    x = _t(r["x"]).permute(0, 2, 1).reshape(K.HEAD_B, K.HEAD_C, 32, 32)
    want = TF.conv2d(TF.silu(TF.group_norm(x, 32, _t(r["gamma"]), _t(r["beta"]), K.EPS)), w4(r["w"]), _t(r["bias"]), padding=1).numpy()
    assert _close(y, want, 1e-7) and (rad > 0).all()                  # (1e-7: the reference divides the folded argument by the float32 constant again)
    lab = _t(K.LABELS)
    a = lab[:, None] * torch.exp(torch.arange(64, dtype=torch.float64) * -K.KC)[None, :]
    assert _close(K.embed_reference()[0], torch.cat([torch.sin(a), torch.cos(a)], dim=1).numpy(), 1e-13)
    assert abs(K.KC - math.log(10000.0) / 63) < 1e-7
    s = K.stem_case()
    cols = TF.unfold(_t(bf16_bits_to_f64(f32_to_bf16_bits(s["x"]))), 3, padding=1)                 # [B][c 9 + tap][1024]
    want = cols.reshape(K.STEM_B, 3, 9, 1024).permute(0, 3, 2, 1).reshape(-1, 27).numpy()
    assert np.array_equal(bf16_bits_to_f64(s["y"][:, :27]), want) and not s["y"][:, 27:].any()
    for q in K.FOLD_QUADS:
        c = K.fold_case(q, 320, 5, False)
        assert _close(c["y"], _t(c["P"]).reshape(K.FOLD_B, 64, 5, q, 2).sum(dim=2).numpy(), 1e-14)
    for case in K.FIN_CASES[:4]:                                      # the exact family's tables are the GroupNorm of its x
        c = K.fin_case(case, "exact")
        assert (c["var"] > 0).all()


# ---- 2. every case reaches the path it is named for --------------------------------------------------------------------------------------------------------------

def test_cases_reach_the_paths_they_name():
    # k_gn_stats: lanes 16 / 8 / 5 / 4, 240 active threads at C = 384, a last ragged round of pixels there (HW % 5 != 0), s_part within its 2112 floats
    assert [K.stats_lanes(C) for C in (128, 256, 384, 512)] == [16, 8, 5, 4]
    assert (384 // 8) * K.stats_lanes(384) == 240 and all(HW % 5 for C, HW in K.STATS_SHAPES if C == 384)
    assert all(K.stats_lanes(C) * C <= 2112 for C in range(32, 513, 32))
    assert {HW for C, HW in K.STATS_SHAPES if C == 512} == {16, 64, 256} and (128, 1024) in K.STATS_SHAPES and (256, 1024) in K.STATS_SHAPES
    c = K.stats_input(256, 64, "one_hot_group")
    g = c["x"][:, :, K.HOT_GROUP * 8:(K.HOT_GROUP + 1) * 8]
    assert np.count_nonzero(g) == K.B and c["x"][0, 63, K.HOT_GROUP * 8 + 7] == 3.0
    c = K.stats_input(256, 64, "mix")
    rms = np.sqrt((c["x"].reshape(K.B, 64, 32, 8) ** 2).mean(axis=(1, 3)))
    assert (np.maximum(rms[:, 1:] / rms[:, :-1], rms[:, :-1] / rms[:, 1:]) > 30).all() and (np.maximum(rms[1:] / rms[:-1], rms[:-1] / rms[1:]) > 30).all()
    assert (K.group_moments(K.stats_input(128, 16, "tiny")["x"], 128)[1] < 3e-5).all()          # the epsilon is a tenth of the variance
    assert K.stats_input(128, 16, "const")["x"].min() == K.CONST_VALUE == bf16_bits_to_f64(f32_to_bf16_bits(F([K.CONST_VALUE])))[0]
    # k_gn_finalize: the clamp var < 0 -> 0 is reached (`const`: the float32 restatement's E[x^2] - mean^2 is negative in some group of some case), one_hot_group as for k_gn_stats
    neg = 0
    for case in K.FIN_CASES:
        c = K.fin_case(case, "const")
        assert (c["var"] == 0).all()
        neg += int((K.fin_unclamped_var(c) < 0).sum())
    assert neg > 0
    # the tail loop (tps % 4 != 0) with and without a four-tile round in front, the second source, a group that spans both sources
    tps = {t for q0, q1, t0, t1, HW in K.FIN_CASES for t in (t0, t1) if t}
    assert tps == {1, 2, 3, 5, 8, 64} and any(t % 4 and t > 4 for t in tps) and any(t < 4 for t in tps) and any(t % 4 == 0 for t in tps)
    assert {(4 * q0, 4 * q1) for q0, q1, *_ in K.FIN_CASES if q1} == {(128, 128), (256, 128), (256, 256)}
    assert all(t0 != t1 and HW % t0 == 0 and (not t1 or HW % t1 == 0) and 4 * (q0 + q1) % 128 == 0 for q0, q1, t0, t1, HW in K.FIN_CASES)
    assert 64 % (384 // 128) != 0                                     # C = 384: quads0 = 64 is no multiple of the 3 quads of a group
    # k_gn_fold: fold < lanes, fold no multiple of lanes, 64 output rows, the VAE's 512 x 512 shape
    lanes = {q: 256 // q for q in K.FOLD_QUADS}
    assert all(256 % q == 0 for q in K.FOLD_QUADS) and all(t // f == 64 for t, f in K.FOLD_SHAPES)
    assert any(f < lanes[32] for _, f in K.FOLD_SHAPES) and any(f % lanes[q] for _, f in K.FOLD_SHAPES for q in K.FOLD_QUADS) and (4096, 64) in K.FOLD_SHAPES
    # k_gn_apply: the ragged last row block of 34 padded rows, 240 threads, lanes beyond the padded width, every value of every switch
    geo = {case: K.apply_geometry(case) for case in K.APPLY_CASES}
    assert any(dp == 34 and dp % K.GN_ROWS == 2 for d, dp, cpp, lanes in geo.values())
    assert any(cpp * lanes == 240 for d, dp, cpp, lanes in geo.values()) and any(lanes > dp for d, dp, cpp, lanes in geo.values())
    assert any(lanes > dp * K.GN_ROWS for d, dp, cpp, lanes in geo.values())                                  # C = 64, side 4, down: lanes past the whole block
    for i, vals in ((2, {0, 1, 2}), (3, {0, 1}), (4, {0, 1}), (5, {0, 1})):
        assert {case[i] for case in K.APPLY_CASES} == vals
    assert {case[0] for case in K.APPLY_CASES} == {64, 128, 384, 512, 256} and {case[1] for case in K.APPLY_CASES} == {4, 8, 32}
    assert any(case[6] > case[0] for case in K.APPLY_CASES) and {(m, bool(x)) for _, _, m, _, _, x, _ in K.APPLY_CASES} >= {(0, True), (1, True), (2, True), (2, False)}
    c = K.apply_case(K.APPLY_CASES[0])
    v = c["x"] * c["scale"].astype(np.float64)[:, None, None, :] + c["shift"].astype(np.float64)[:, None, None, :]
    assert v.max() == K.BIG_V and v.min() == -K.BIG_V
    assert np.abs(c["x"][c["x"] != 0]).min() < 2.0 ** -126 and np.signbit(c["x"][0, 0, 1, 0]) and c["x"][0, 0, 1, 0] == 0      # bf16 sub-normals, -0
    wide = K.apply_case(K.APPLY_CASES[1])["xbits"]
    assert wide.shape[-1] == 192 and (bf16_bits_to_f64(wide[..., 128:]) > 9e3).all()                          # the other channels of a wider row hold 1e4
    act_shift = np.abs(K._silu64(c["shift"].astype(np.float64)))
    assert act_shift.min() > 7e-3                                     # a border that holds act(shift) is no zero
    # k_head_conv: both halves, nine taps, three output channels; t = 0 and |t| = 100
    assert {c >> 6 for c, _, _ in K.ONE_HOT} == {0, 1} and {t for _, t, _ in K.ONE_HOT} == set(range(9)) and {n for _, _, n in K.ONE_HOT} == {0, 1, 2}
    o = K.head_onehot_case()
    hot_ch = [ch for ch, _, _ in K.ONE_HOT]
    assert 3 in hot_ch and (o["t"][..., 3] == 0).any() and o["t"][..., hot_ch].max() > 99 and o["t"][..., hot_ch].min() < -99
    assert sorted(K.head_k(np.arange(128)[:, None], np.arange(9)[None, :]).ravel().tolist()) == list(range(K.HEAD_K))
    assert (bf16_bits_to_f64(K.head_exact_case()["w16"][3:]) > 9e3).all()                                     # rows 3 .. 15 of the weight buffer: bf16(1e4)
    # glue: the pack forms address what they say; the stem's four edges hold zeros
    f1, f2, f3, f4 = (K.pack_form_case(f)["y"] for f in K.PACK_FORMS)
    assert (f1 != K.SENTINEL).all() and (f2[:, 27:] == K.SENTINEL).all() and (f2[:, :27] != K.SENTINEL).all()
    assert (f3[:, :1152] == K.SENTINEL).all() and (f3[:, 1152:] != K.SENTINEL).all() and (f4 != K.SENTINEL).all()
    y = K.stem_case()["y"].reshape(K.STEM_B, 32, 32, 64)
    assert not y[:, 0, :, 0:9].any() and not y[:, 31, :, 18:27].any() and not y[:, :, 0, 0:3].any() and not y[:, :, 31, 6:9].any() and y[:, 1:31, 1:31, :27].all()
    n = K.nchw_case()["x"]
    assert ((n & 0x7f80) == 0).any() and ((n & 0x7f80) != 0x7f80).all()
    assert K.TRANSPOSE_CASE[0] != K.TRANSPOSE_CASE[1] and K.TRANSPOSE_CASE[2] > K.TRANSPOSE_CASE[0] and K.NCHW_CASE[3] > K.NCHW_CASE[2]


# ---- 3. the float32 restatements pass, 4. the mutants fail -------------------------------------------------------------------------------------------------------

def test_restated_gn_stats_passes_and_mutants_fail():
    worst = 0.0
    for C, HW in K.STATS_SHAPES:
        for fam in K.STATS_FAMILIES:
            c = K.stats_input(C, HW, fam)
            for om in K.OUT_MULS:
                bad, ratio = K.check_table(K.stats_interval(C, HW, fam, om), *K.stats_restated(c, om))
                assert bad == 0, (c["name"], om, ratio)
                worst = max(worst, ratio)
    print(f"\nk_gn_stats restated: worst error / radius = {worst:.3f}")
    assert worst < 1.0
    # each mutant on the family it rests on (module docstring of the cases: the epsilon shows on `randn` and `tiny` only)
    on = {"eps_1e-5": ("randn", "tiny"), "unbiased_variance": ("randn",), "group_size+1": ("randn", "mix"), "group_size-1": ("randn", "mix"),
          "out_mul_on_scale_only": ("randn", "const"), "mean_over_HW": ("mean8", "const")}
    for mutant in K.STATS_MUTANTS:
        for fam in on[mutant]:
            # (at the longest chain, C = 256 with HW = 1024, L = 148 and the radius has grown to the size of the epsilon's effect on `randn`: there it rests on `tiny`)
            for C, HW in ((128, 16), (384, 64), (512, 256)) + (((256, 1024),) if (mutant, fam) != ("eps_1e-5", "randn") else ()):
                c = K.stats_input(C, HW, fam)
                om = K.NEG_LOG2E if mutant == "out_mul_on_scale_only" else 1.0
                bad, ratio = K.check_table(K.stats_interval(C, HW, fam, om), *K.stats_restated(c, om, mutant))
                assert bad > 0, (mutant, c["name"])
                if mutant == "eps_1e-5":
                    print(f"eps 1e-5 on {c['name']}: {ratio:.3g} radii")
                    assert ratio > (1e4 if fam == "tiny" else 1.2)


def test_restated_gn_finalize_passes_and_mutants_fail():
    worst, worst_exact = 0.0, 0.0
    for case in K.FIN_CASES:
        for fam in K.FIN_FAMILIES:
            c = K.fin_case(case, fam)
            for om in K.OUT_MULS:
                iv, got = K.fin_interval(c, om), K.fin_restated(c, om)
                bad, ratio = K.check_table_exact(iv, *got) if fam == "exact" else K.check_table(iv, *got)
                assert bad == 0, (c["name"], om, ratio)
                if fam == "exact": worst_exact = max(worst_exact, ratio)
                else: worst = max(worst, ratio)
    print(f"\nk_gn_finalize restated: worst error / radius = {worst:.3f}; exact tables: worst error / (1e-5 max |table|) = {worst_exact:.4f}")
    on = {"eps_1e-5": ("randn", "tiny"), "unbiased_variance": ("randn",), "out_mul_on_scale_only": ("randn", "const"), "tail_tiles_dropped": ("randn", "exact"),
          "second_source_offset_by_quads0": ("mix", "exact"), "sample_stride_of_source0": ("mix", "exact")}
    for mutant in K.FIN_MUTANTS:
        for fam in on[mutant]:
            cases = [cs for cs in K.FIN_CASES if (cs[1] if "source" in mutant else True) and (cs[2] % 4 if mutant == "tail_tiles_dropped" else True)]
            for case in cases:
                c = K.fin_case(case, fam)
                om = K.NEG_LOG2E if mutant == "out_mul_on_scale_only" else 1.0
                iv, got = K.fin_interval(c, om), K.fin_restated(c, om, mutant)
                bad, _ = K.check_table_exact(iv, *got) if fam == "exact" else K.check_table(iv, *got)
                assert bad > 0, (mutant, c["name"])


def test_stats_and_finalize_agree_on_the_same_x():
    """k_gn_stats on x and k_gn_finalize on the fp64-summed quad partials of the same x: each restated table inside the other kernel's interval"""
    for C, HW, tps in ((128, 64, 2), (256, 256, 8), (384, 64, 4), (512, 16, 1)):
        c = K.stats_input(C, HW, "randn")
        fc, iv_f = K.fin_from_x(c, tps)
        for om in K.OUT_MULS:
            iv_s = K.stats_interval(C, HW, "randn", om)
            t_s, t_f = K.stats_restated(c, om), K.fin_restated(fc, om)
            bad_sf, r_sf = K.check_table(iv_f(om), *t_s)
            bad_fs, r_fs = K.check_table(iv_s, *t_f)
            print(f"\nC{C} HW{HW} tps{tps} out_mul {om:.3f}: stats in finalize's interval {r_sf:.3f}, finalize in stats' interval {r_fs:.3f}")
            assert bad_sf == 0 and bad_fs == 0


def test_restated_gn_fold_passes_and_mutants_fail():
    worst = 0.0
    for q in K.FOLD_QUADS:
        for tps, fold in K.FOLD_SHAPES:
            for exact in (True, False):
                c = K.fold_case(q, tps, fold, exact)
                bad, ratio = K.check_fold(c, K.fold_restated(c))
                assert bad == 0, c["name"]
                worst = max(worst, ratio)
                for mutant in K.FOLD_MUTANTS:
                    assert K.check_fold(c, K.fold_restated(c, mutant))[0] > 0, (mutant, c["name"])
    print(f"\nk_gn_fold restated: worst error / radius = {worst:.3f}")


def test_restated_gn_apply_passes_and_mutants_fail():
    worst = 0.0
    for case in K.APPLY_CASES:
        c = K.apply_case(case)
        bad, ratio = K.check_apply(c, *K.apply_restated(c))
        assert bad == 0, (c["name"], ratio)
        worst = max(worst, ratio)
    print(f"\nk_gn_apply restated: worst (|k - y| - half ulp) / delta = {worst:.3f}")
    on = {"border_holds_act_shift": lambda cs: cs[3] == 1, "up_shift_before_pad": lambda cs: cs[2] == K.RS_UP and cs[3] == 1,
          "down_three_taps": lambda cs: cs[2] == K.RS_DOWN, "down_rounds_each_term": lambda cs: cs[2] == K.RS_DOWN,
          "table_chunk_from_swapped_lane": lambda cs: cs[0] == 384, "scale_of_sample_0": lambda cs: True}
    for mutant in K.APPLY_MUTANTS:
        cases = [cs for cs in K.APPLY_CASES if on[mutant](cs)]
        assert cases
        for case in cases:
            c = K.apply_case(case)
            assert K.check_apply(c, *K.apply_restated(c, mutant))[0] > 0, (mutant, c["name"])


def test_restated_head_conv_passes_and_mutants_fail():
    e = K.head_exact_case()
    run = lambda c, w16, bias, m=None: K.head_restated(c["x"], c["scale"], c["shift"], w16, bias, m)
    assert np.array_equal(run(e, e["w16"], e["bias"]).astype(np.float64), e["y"])
    for mutant in ("dx_dy_swapped", "halves_swapped", "border_not_zeroed", "bias_per_pixel_tile"):
        assert not np.array_equal(run(e, e["w16"], e["bias"], mutant).astype(np.float64), e["y"]), mutant
    o = K.head_onehot_case()
    worst = 0.0
    for hot in K.ONE_HOT:
        w16 = K.head_pack(K.onehot_weights(*hot))
        bad, ratio = K.check_head_onehot(o, hot, run(o, w16, np.zeros(3, F)))
        assert bad == 0, hot
        worst = max(worst, ratio)
        for mutant in ("dx_dy_swapped", "halves_swapped") + (("border_not_zeroed",) if hot[1] != 4 and hot[0] != 3 else ()):      # (channel 3 has shift 0: g(shift) = 0)
            if mutant == "dx_dy_swapped" and hot[1] in (0, 4, 8):
                continue                                              # the diagonal taps are their own transposes
            assert K.check_head_onehot(o, hot, run(o, w16, np.zeros(3, F), mutant))[0] > 0, (mutant, hot)
    print(f"\nk_head_conv restated, one-hot: worst (|k - g| - half ulp) / dg = {worst:.3f}")
    r = K.head_random_input()
    y, rad, iv = K.head_random_reference()
    tables = K.stats_restated(dict(C=K.HEAD_C, HW=1024, x=_pad_batch(r["x"]), gamma=r["gamma"], beta=r["beta"]), K.NEG_LOG2E)
    sc, sh = tables[0][:K.HEAD_B], tables[1][:K.HEAD_B]
    xv = r["x"].reshape(K.HEAD_B, 32, 32, K.HEAD_C)
    for mutant in (None, "weights_without_ln2"):
        w16 = K.head_pack((r["w"] if mutant else (r["w"] * K.NEG_LN2_F).astype(F)))
        bad, ratio = K.check_head_random(y, rad, K.head_restated(xv, sc, sh, w16, r["bias"]))
        print(f"k_head_conv restated, random ({mutant}): worst error / radius = {ratio:.3f}")
        assert (bad > 0) == (mutant is not None)


def _pad_batch(x):
    """stats_restated works on K.B samples: repeat the last one"""
    return np.concatenate([x] + [x[-1:]] * (K.B - x.shape[0]))


def test_restated_glue_kernels_and_mutants():
    bad, ratio, pyth = K.check_embed(K.embed_restated())
    print(f"\nk_time_embed restated: worst (|k - y| - half ulp) / delta = {ratio:.3f}, |sin^2 + cos^2 - 1| / bound = {pyth:.3f}")
    assert bad == 0
    big = np.resize(K.LABELS, 40)                                    # check_embed with labels of the caller (the GPU test's B = 8200 form)
    assert K.check_embed(np.resize(K.embed_restated(), (40, 128)), big)[0] == 0 and K.BIG_BATCH * 128 > 4096 * 256
    for mutant in K.EMBED_MUTANTS:
        assert K.check_embed(K.embed_restated(mutant))[0] > 0, mutant
    s = K.stem_case()
    for mutant in ("dx_dy_swapped", "channel_major"):
        assert not np.array_equal(K.stem_reference(s["x"], mutant), s["y"])
    form = K.PACK_FORMS[0]
    c = K.pack_form_case(form)
    assert not np.array_equal(K.pack_conv_reference(c["src"], np.full_like(c["y"], K.SENTINEL), *form, drop_wmul=True), c["y"])


# ---- 5. the exact families are exact -----------------------------------------------------------------------------------------------------------------------------

def test_exact_families_are_exact():
    for case in K.FIN_CASES:
        c = K.fin_case(case, "exact")
        for P in (c["P0"], c["P1"]):
            if P is not None:
                assert np.array_equal(P * 4, np.rint(P * 4))
        assert c["max_sum"] * 4 < 2 ** 24 and c["max_sum"] < 2 ** 22
    for q in K.FOLD_QUADS:
        for tps, fold in K.FOLD_SHAPES:
            c = K.fold_case(q, tps, fold, True)
            assert np.array_equal(c["P"] * 4, np.rint(c["P"] * 4)) and c["max_sum"] * 4 < 2 ** 24
    e = K.head_exact_case()
    assert set(np.unique(e["t"]).tolist()) == {-40.0, -48.0, -56.0, -64.0} and np.array_equal(bf16_bits_to_f64(f32_to_bf16_bits(e["t"].astype(F))), e["t"])
    assert (F(1.0) + np.exp2(e["t"].astype(F)) == F(1.0)).all()      # 1 + 2^t is 1 in fp32: the activation is t itself
    assert set(np.unique(e["w"]).tolist()) == {-1.0, -0.5, 0.0, 0.5, 1.0} and e["max_sum"] * 2 < 2 ** 24 and np.array_equal(e["y"] * 2, np.rint(e["y"] * 2))
    assert np.array_equal(bf16_bits_to_f64(e["w16"][:3]).reshape(3, 2, 9, 64).transpose(0, 1, 3, 2).reshape(3, 128, 9), e["w"])
