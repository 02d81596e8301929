"""The comparators of tests/glue_kernel_cases.py are attainable and discriminating, shown on the CPU before a GPU is involved: a numpy-float32 restatement of every
glue kernel, in the kernel's own order, passes every case that tests/test_gpu_glue_kernels.py runs, and each mutant -- the slips that the whole-network
tolerances of 3e-2 / 4e-2 let through -- fails a case named here."""
import numpy as np
import pytest

import glue_kernel_cases as G

F = np.float32


def _patch_run(c, half, guard, mutant=None, plain=None):
    x, slot = G.patch_restated(c, half, guard, mutant)
    K, D = c["K"], c["D"]
    wt = np.concatenate([[np.nan], (G.transpose_restated(c["w"]) if mutant != "transpose_skipped" else c["w"].reshape(K, D)).ravel(), [np.nan]]).astype(F)
    return G.check_patch(c, half, x, wt, slot, plain), x


def test_number_format_helpers():
    x = G.SPECIAL_F32
    bits = G.f32_to_bf16_bits(x)
    assert not G.check_bf16_bytes(G.bf16_expected_bits(x), bits, np.isnan(x))                  # the value statement and the bit trick agree, specials included
    assert bits[:8].tolist() == [0x3f80, 0x3f82, 0xbf80, 0xbf82, 0x3f81, 0x3f80, 0x8000, 0x0000]            # ties to even both ways, just off a tie, the zeros
    assert bits[8:14].tolist() == [0x0001, 0x0000, 0x0002, 0x0001, 0x8002, 0x0080]                          # sub-normals: a tie to zero, a tie to 2, the smallest normal from below
    assert bits[14:20].tolist() == [0x7f80, 0xff80, 0x7f7f, 0x7f80, 0x7f80, 0xff80]                         # the largest finite fp32 -> inf; 0x7f7f8000 is a tie to inf
    assert G.is_bf16_nan(bits[20:]).all() and not G.is_bf16_nan(bits[:20]).any()
    assert G.check_bf16_bytes(G.bf16_expected_bits(x), G.f32_to_bf16_bits(x, truncate=True), np.isnan(x))  # truncation shows on the specials alone
    assert G.rne_half([65519.9, 65520.0, 2049.0, 2051.0, -7e4]).tolist() == [65504.0, np.inf, 2048.0, 2052.0, -np.inf]
    assert G.half_ulp_half([1.0, 2048.0, 1e-7]).tolist() == [2.0 ** -11, 1.0, 2.0 ** -25]
    r = np.random.default_rng(0).standard_normal(4096).astype(F) * 7
    assert np.array_equal(G.f32_to_bf16_bits(r), G.R.f32_to_bf16_bits(r))


def test_cases_reach_every_path():
    assert len(G.patch_case_ids()) == 24
    for C, g, B, D in G.patch_case_ids():
        c = G.patch_case(C, g, B, D)
        assert np.abs(c["y"]).max() < 10000 and np.all(c["y"] == np.rint(c["y"])) and np.all(c["bias"] != 0)
        assert (c["rows"] % G.PE_TOK != 0) == (g == 3) and c["K"] <= 64
    assert {4 * C for C in G.PATCH_C} == {4, 16, 64} and all(D % 64 == 0 and D * 4 * C % 256 == 0 for D in G.PATCH_D for C in G.PATCH_C)
    o = G.patch_case(*G.OVERFLOW_CASE, overflow=True)
    assert np.all(o["y"][:, G.OVERFLOW_CH] > 65520) and np.abs(np.delete(o["y"], G.OVERFLOW_CH, axis=1)).max() < 2000
    for R_ in G.IMAGES_R:
        c = G.images_case(R_)
        assert np.any(c["img"].view(np.uint32) == 0x80000000) and (R_ == 1 or (c["nan"].any() and np.any(c["bits"] == 0x7f80)))
    for C in G.LATENTS_C:
        for r_ in G.LATENTS_R:
            c = G.latents_case(C, r_)
            assert c["interior"].sum() == G.VAE_B * r_ * r_ * C and (C < 4 or np.all(np.signbit(c["y"][:, 1, 1, C - 1])))
    assert np.isnan(G.cond_case(64)["table"]).sum() == (G.COND_CLASSES - 3) * 64
    assert G.time_case(7)["t"].tolist() == [F(v) for v in G.TIME_STEPS] and set(G.time_case(3)["t"].tolist()) <= set(G.time_case(7)["t"].tolist())
    assert -(-G.TIME_B[-1] * 256 // 256) > 4096 and -(-G.COND_LARGE[0] * G.COND_LARGE[1] // 256) > 4096 > -(-G.COND_LARGE[0] * 910 // 256)      # past the old grid cap


def test_restated_patch_embed_passes():
    """all 24 shapes x {fp32, half} x {plain, guarded}, and the overflow case: guarded bytes = plain bytes, count 0, the maximum's bit pattern"""
    worst = 0.0
    for cid in G.patch_case_ids():
        c = G.patch_case(*cid)
        for half in (False, True):
            (fails, ratio), plain = _patch_run(c, half, False)
            assert not fails, (c["name"], half, fails)
            (fails, r2), _ = _patch_run(c, half, True, plain=plain)
            assert not fails, (c["name"], half, "guarded", fails)
            worst = max(worst, ratio, r2)
    o = G.patch_case(*G.OVERFLOW_CASE, overflow=True)
    for guard in (False, True):
        (fails, _), _ = _patch_run(o, True, guard)
        assert not fails, (guard, fails)
    print(f"\nrestated k_patch_embed: worst (|x - y| - half an output ulp) / delta = {worst:.3f} (integer inputs: the fp32 sums are exact)")
    assert worst == 0.0


# mutant -> (case, half stream, guarded): a case where it must fail
PATCH_MUTANT_CASES = {
    "taps_exchanged": ((4, 4, 2, 64), False, False),
    "pos_row_from_block": ((4, 3, 3, 320), True, False),            # g = 3: a sample ends at row 9, inside the first block
    "tail_writes_neighbour": ((16, 3, 3, 1536), False, False),      # 27 rows: the block's rows 27.. land on the canary row
    "bias_dropped": ((1, 4, 2, 1152), True, True),
    "transpose_skipped": ((16, 4, 2, 64), False, False),            # W[d][k] read where Wt[k][d] is meant
}


@pytest.mark.parametrize("mutant", list(PATCH_MUTANT_CASES))
def test_patch_mutants_fail(mutant):
    cid, half, guard = PATCH_MUTANT_CASES[mutant]
    c = G.patch_case(*cid)
    (fails, _), _ = _patch_run(c, half, guard, mutant)
    assert fails, mutant
    (fails, _), _ = _patch_run(c, half, guard)
    assert not fails


def test_pos_row_mutant_fails_after_the_sample_boundary_only():
    c = G.patch_case(4, 3, 3, 64)
    x, _ = G.patch_restated(c, False, False, "pos_row_from_block")
    wrong = np.nonzero(np.any(x[1:-1].astype(np.float64) != c["y"], axis=1))[0]
    assert wrong.min() == 9 and set(wrong.tolist()) <= set(range(9, 16)) | set(range(18, 27))       # block 0 goes wrong at row 9 (t = 0 again), block 1 at row 18


def test_guard_mutant_and_overflow_contract():
    o = G.patch_case(*G.OVERFLOW_CASE, overflow=True)
    x, slot = G.patch_restated(o, True, True)
    assert slot[1] == o["rows"] and np.all(x[1:-1, G.OVERFLOW_CH] == 0x7bff)                         # 65,504, counted once per row
    xp, _ = G.patch_restated(o, True, False)
    assert np.all(xp[1:-1, G.OVERFLOW_CH] == 0x7c00)                                                 # the bare cast: IEEE inf
    (fails, _), _ = _patch_run(o, True, True, "clamp_not_counted")
    assert any("count" in f for f in fails)
    # a guarded result handed to the unguarded expectation and the other way round both fail
    assert G.check_patch(o, True, x)[0] and G.check_patch(o, True, xp, slot=slot)[0]


def test_restated_data_movement_passes_and_its_mutants_fail():
    for OC in G.UNPATCH_OC:
        for g in G.UNPATCH_G:
            c = G.unpatch_case(OC, g)
            assert np.array_equal(G.unpatch_restated(c).view(np.uint32), c["out"].view(np.uint32)), (OC, g)
            assert not np.array_equal(G.unpatch_restated(c, "c_and_taps_swapped"), c["out"]), (OC, g)       # every shape catches it (OC > 1)
    for n in G.CAST_N:
        c = G.cast_case(n)
        assert not G.check_bf16_bytes(c["bits"], G.f32_to_bf16_bits(c["x"]), c["nan"]), n
        assert G.check_bf16_bytes(c["bits"], G.f32_to_bf16_bits(c["x"], truncate=True), c["nan"]), n
    for R_ in G.IMAGES_R:
        c = G.images_case(R_)
        assert not G.check_bf16_bytes(c["bits"], G.images_restated(c), c["nan"]), R_
        assert G.check_bf16_bytes(c["bits"], G.images_restated(c, "border_minus_zero"), c["nan"]), R_
    assert G.check_bf16_bytes(G.images_case(17)["bits"], G.images_restated(G.images_case(17), "bf16_truncated"), G.images_case(17)["nan"])
    for C in (1, 4, 16):
        w = G.patch_case(C, 4, 2, 64)["w"]
        assert np.array_equal(G.transpose_restated(w), w.T)


def test_restated_vae_chains_pass_and_their_mutants_fail():
    worst_l = worst_q = 0.0
    for C in G.LATENTS_C:
        for r_ in G.LATENTS_R:
            c = G.latents_case(C, r_)
            fails, ratio = G.check_latents(c, G.latents_restated(c))
            assert not fails, (C, r_, fails)
            worst_l = max(worst_l, ratio)
            assert G.check_latents(c, G.latents_restated(c, "border_minus_zero"))[0], (C, r_)
            if C > 1:
                assert G.check_latents(c, G.latents_restated(c, "W_transposed"))[0], (C, r_)
    assert G.check_latents(G.latents_case(64, 8), G.latents_restated(G.latents_case(64, 8), "bf16_truncated"))[0]
    for N in G.QUANT_N:
        for hw in G.QUANT_HW:
            c = G.quant_case(N, hw)
            bad, ratio = G.check_interval(c["y"], c["delta"], G.quant_restated(c), "f32")
            assert not bad, (N, hw)
            worst_q = max(worst_q, ratio)
            assert G.check_interval(c["y"], c["delta"], G.quant_restated(c, "W_transposed"), "f32")[0], (N, hw)
    print(f"\nrestated k_vae_latents: worst (|y16 - y| - half ulp) / delta = {worst_l:.3f}; restated k_vae_quant: worst |out - y| / delta = {worst_q:.3f}")
    assert worst_l < 1.0 and worst_q < 1.0          # (k_vae_quant's worst is at N = 2: four roundings against a radius of three units, nothing to spare by design)


TIME_MUTANTS = ("sin_cos_order", "h_over_127", "max_period_1e3")


def test_restated_transcendentals_pass_and_their_mutants_fail():
    worst = {}
    for B in G.TIME_B:
        c = G.time_case(B)
        bits, v = G.time_restated(c)
        bad, ratio = G.check_interval(c["y"], c["delta"], G.bf16_bits_to_f64(bits), "bf16")
        assert not bad, (B, bad[:4])
        raw = float(np.max(np.abs(v.astype(np.float64) - c["y"])[c["delta"] > 0] / c["delta"][c["delta"] > 0]))
        worst["k_dit_time_freq"] = max(worst.get("k_dit_time_freq", 0.0), raw)
        for m in TIME_MUTANTS:
            assert G.check_interval(c["y"], c["delta"], G.bf16_bits_to_f64(G.time_restated(c, m)[0]), "bf16")[0], (B, m)
        z = np.nonzero(c["t"] == 0)[0]
        assert np.all(bits[z, :128] == 0x3f80) and np.all(bits[z, 128:] == 0)                       # t = 0: cos 1, sin 0, radius 0
    for n in G.SILU_N:
        c = G.silu_case(n)
        v = G.silu_restated(c["x"])
        bad, _ = G.check_interval(c["y"], c["delta"], G.bf16_bits_to_f64(G.f32_to_bf16_bits(v)), "bf16")
        assert not bad, (n, bad[:4])
        worst["k_silu_bf16"] = max(worst.get("k_silu_bf16", 0.0), float(np.max(np.abs(v.astype(np.float64) - c["y"]) / c["delta"])))
        if n > 1:
            assert G.check_interval(c["y"], c["delta"], G.bf16_bits_to_f64(G.f32_to_bf16_bits(v, truncate=True)), "bf16")[0], n
    for D, B in [(D, G.COND_B) for D in G.COND_D] + [G.COND_LARGE]:
        c = G.cond_case(D, B)
        v = G.cond_restated(c)
        bad, _ = G.check_interval(c["y"], c["delta"], G.bf16_bits_to_f64(G.f32_to_bf16_bits(v)), "bf16")
        assert not bad, (D, bad[:4])
        worst["k_dit_cond"] = max(worst.get("k_dit_cond", 0.0), float(np.max(np.abs(v.astype(np.float64) - c["y"]) / c["delta"])))
        m = G.bf16_bits_to_f64(G.f32_to_bf16_bits(G.cond_restated(c, "null_row_off_by_one")))
        bad, _ = G.check_interval(c["y"], c["delta"], m, "bf16")
        assert bad and set(i // D for i in bad) == set(range(2, B, 3)), D                            # the samples with the null class, and only they (row 9 is NaN)
    print("\nrestated transcendentals, worst |fp32 value - y| / radius: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0                # (SiLU at large s is two roundings against a radius of two units: tight by design)
