"""Inputs, fp64 references, radii and comparators for the glue kernels at the two ends of the DiT, SD3-MMDiT and AutoencoderKL engines, tested alone
(tests/test_glue_kernels_host.py on the CPU, tests/test_gpu_glue_kernels.py on the GPU): k_patch_embed<XH, GUARD> with the load-time transpose k_transpose_f32,
k_dit_time_freq, k_dit_cond, k_silu_bf16, k_f32_to_bf16, k_unpatchify (csrc/transformer_rows.h, csrc/engine_core.h), k_vae_latents, k_vae_images
(csrc/vae_engine.inc) and k_vae_quant (csrc/vae_quant.hip).  numpy only.

References are restated from the operation, never from a kernel: the patch embedding is Conv2d(C, D, 2, stride 2) flattened plus the positional table; the time
embedding is DiT's timestep_embedding (models.py:41-58: half = 128, freqs = exp(-ln(1e4) arange(half) / half), [cos | sin]; diffusers' Timesteps(flip_sin_to_cos =
True, downscale_freq_shift = 0) is the same); unpatchify is models.py:222-235 (reshape to (N, h, w, p, p, c), einsum nhwpqc -> nchpwq); the VAE passes are 1x1
convolutions and the NHWC zero-bordered 64-channel layout csrc/vae_engine.inc documents.

u = 2^-24 is the unit roundoff of fp32.  Three kinds of bound:

(1) Pure data movement, compared as BYTES: k_unpatchify, k_transpose_f32, k_f32_to_bf16, k_vae_images, and the zero border / spare channels of k_vae_latents.
    bf16 is round to nearest even; a NaN must stay a NaN (any payload); beyond the largest finite bf16, inf.

(2) fp32 chains (k_patch_embed, k_vae_latents, k_vae_quant): y = b + sum_{k < K} w_k v_k (+ pos).  A correct fp32 kernel rounds every product once and every
    addition once, fused or not; a term passes through its product's rounding and at most K (+ 1 with pos) additions, so
        delta = (K + 2) u (|b| + sum |w_k v_k| + |pos|)      patch embedding, K = 4 C
        delta = (K + 1) u (|b| + sum |w_k v_k|)              k_vae_latents (K = C), k_vae_quant (K = N)
    fp32 outputs lie within delta; bf16 / half outputs within [rne(y - delta), rne(y + delta)].  The patch embedding's inputs are integers of a few magnitudes: every
    partial sum is an integer below 2^24, the fp32 result is exact, and a wrong tap, channel, token or table row moves an element by whole units.

(3) Transcendentals.  Analytic parts, from the code:
    k_dit_time_freq: a = fl(t * expf(q)), q = fl(c32 * h) / 128 with c32 = float32(-ln 1e4) (relative error <= u), the product one rounding (u), the division by 128
    exact: q = e (1 + theta), |theta| <= 2u, e = -ln(1e4) h / 128, |e| <= 9.14.  The exponential turns that into a RELATIVE error 2u |e| of the frequency; the product
    with t adds u: rho = (2 |e| + 1) u <= 19.3 u, and with expf itself at one ulp (2u) 21.3 u -- the "about 22" that matters at a = 1,000 (1.3e-3 absolute, next to
    a bf16 half-ulp of 1.95e-3).  |d cos| and |d sin| are at most |a| rho.
    silu_f(s) = s / (1 + __expf(-s)), __expf(x) = exp2(fl(x log2 e)): the rounded product puts u |x| log2(e) into the exponent of two, a relative error u |x| ln 2 log2 e
    = u |s| of E = e^-s; the constant log2 e adds u |s| more.  1 + E is one rounding, the IEEE division another: relative radius u (2 + w (2 |s| + dev)), w = E / (1 + E).
    k_dit_cond first rounds s = c0 + table (u |s|, through |SiLU'| <= 1.1).  Results below 2^-126 may be flushed: FLOOR.
    Device functions (expf, cosf, sinf, __expf) are not this project's numbers.  The ROCm tree the library is built with states no error bound for them (its only
    mention of ulps is the 8192 of OpenCL's half_ functions), so the allowances START from the public OpenCL C full-profile bounds that its device library is written
    to -- exp 3 ulp, sin / cos 4 ulp -- and the instruction set's 1 ulp for v_exp_f32:
        TIME_DEV  = |a| * 3 * 2u + 4 * 2u          (expf inside the argument, cosf / sinf on the result, |result| <= 1)
        SILU_DEV  = 1 * 2u, relative to E          (dev above)
    and are then held against the MI355X: the worst part of |value - fp64 reference| that neither the output's own rounding (half a bf16 ulp) nor the ANALYTIC part
    explains, per kernel family, over every case.  Measured: time embedding 0 (every output lies inside the analytic radius plus its rounding: through a bf16 output nothing
    of the device functions' error shows), SiLU / cond 0 likewise (TIME_MEASURED, SILU_MEASURED; tests/test_gpu_glue_kernels.py prints them per case).  Twice zero leaves no room
    for the rounding these functions certainly have, so the allowances stay at the starting bounds: a smaller one would reject a valid expansion of another compiler.  With them
    every mutant of tests/test_glue_kernels_host.py still fails.
"""
import functools

import numpy as np

import row_kernel_cases as R

U = 2.0 ** -24
F = np.float32
FLOOR = 2.0 ** -126
LN1E4 = float(np.log(1e4))
BF16_CANARY = 0x7fc0

rne_bf16, bf16_bits_to_f64, half_ulp_bf16 = R.rne_bf16, R.bf16_bits_to_f64, R.half_ulp_bf16


def _ro(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---- number formats ----------------------------------------------------------------------------------------------------------------------------------------------

def bf16_value_to_bits(v):
    """fp64 values that ARE bf16 values (or +-inf, +-0) -> their bits"""
    return (np.asarray(v, np.float64).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_expected_bits(x):
    """the operation `round fp32 to the nearest bf16, ties to even` stated on values (R.rne_bf16), as bits; a NaN input is marked by 0x7fc0 and compared by check_bf16_bytes as
    `any NaN`"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        b = bf16_value_to_bits(rne_bf16(np.where(np.isnan(x), 0.0, x).astype(np.float64)))
    return np.where(np.isnan(x), np.uint16(0x7fc0), b).astype(np.uint16)


def f32_to_bf16_bits(x, truncate=False):
    """what `(bf16)float` compiles to, on bits: + 0x7fff + lsb, >> 16; a NaN keeps its top bits and gets the quiet bit.  truncate: a mutant."""
    w = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (w >> 16) if truncate else ((w + 0x7fff + ((w >> 16) & 1)) >> 16)
    nan = (w & 0x7fffffff) > 0x7f800000
    return np.where(nan, (w >> 16) | 0x40, r).astype(np.uint16)


def is_bf16_nan(bits):
    b = np.asarray(bits, np.uint16)
    return (b & 0x7fff) > 0x7f80


def check_bf16_bytes(expected, got, nan_mask=None):
    """bytes equal, except where the input was NaN: there any NaN pattern.  Returns the flat indices that fail."""
    expected, got = np.asarray(expected, np.uint16).ravel(), np.asarray(got, np.uint16).ravel()
    ok = expected == got
    if nan_mask is not None:
        m = np.asarray(nan_mask, bool).ravel()
        ok = np.where(m, is_bf16_nan(got), ok)
    return np.nonzero(~ok)[0].tolist()


def rne_half(v):
    """fp64 -> the nearest IEEE half (ties to even; beyond 65520 inf), as fp64"""
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def half_ulp_half(v):
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))
    return np.exp2(np.maximum(e - 1, -14).astype(np.float64) - 11)


def check_interval(y, delta, k, fmt):
    """k (fp64 values of what a kernel wrote) inside delta (fmt "f32") or inside [rne(y - delta), rne(y + delta)] (fmt "bf16" / "f16"): every element, a NaN fails.
    Returns (flat indices that fail, worst (|k - y| - half an output ulp) / delta over delta > 0)."""
    y, delta, k = (np.asarray(a, np.float64) for a in (y, delta, k))
    if fmt == "f32":
        ok, half = np.abs(k - y) <= delta, 0.0
    else:
        rne, hu = (rne_bf16, half_ulp_bf16) if fmt == "bf16" else (rne_half, half_ulp_half)
        ok, half = (k >= rne(y - delta)) & (k <= rne(y + delta)), hu(k)
    m = (delta > 0) & np.isfinite(k) & np.isfinite(y)
    with np.errstate(invalid="ignore"):
        ratio = float(np.max(np.maximum(np.abs(k - y) - half, 0.0)[m] / delta[m])) if m.any() else 0.0
    return np.nonzero(~ok.ravel())[0].tolist(), ratio


# ---- patch embedding + the load-time transpose ----------------------------------------------------------------------------------------------------------------

PE_TOK = 16
PATCH_C = (1, 4, 16)                    # 16: SD3, C * 4 = 64 fills the kernel's LDS row exactly
PATCH_GB = ((3, 3), (4, 2))             # (g, B): 27 rows -- a clamped tail block, two sample boundaries inside a block -- and 32 rows, exact blocks
PATCH_D = (64, 320, 1152, 1536)         # one live wave; a second block with one live wave; DiT-XL; SD3
Z_SET = np.array([0, 1, -1, 2, -2, 5, -5, 17, -17], np.float64)
W_SET = np.array([0, 1, -1, 3, -3, 7, -7], np.float64)
HALF_MAX = 65504.0
OVERFLOW_CASE = (1, 3, 3, 64)           # the extra half-stream case: C, g, B, D; bias 7e4 on channel OVERFLOW_CH
OVERFLOW_CH = 5


def patch_case_ids():
    return [(C, g, B, D) for C in PATCH_C for g, B in PATCH_GB for D in PATCH_D]


@functools.lru_cache(maxsize=None)
def patch_case(C, g, B, D, overflow=False):
    """z [B][C][2g][2g], w [D][C*4] (the checkpoint's conv weight, flattened), bias [D], pos [g*g][D]: integers as fp32; y fp64 [B*g*g][D] and its radius.
    |y| <= 64 * 17 * 7 + 50 + 400 = 8,066: inside the half range (the overflow case: |y - 7e4| <= 4 * 119 + 400 on its channel, so every value there is above 65,520)."""
    r = np.random.default_rng(100000 * C + 1000 * g + 10 * D + B + (7 if overflow else 0))
    K, T, S = 4 * C, g * g, 2 * g
    z = r.choice(Z_SET, (B, C, S, S))
    w = r.choice(W_SET, (D, K))
    bias = r.integers(-50, 51, D).astype(np.float64)
    bias[bias == 0] = 13.0                                       # (a dropped bias must show in every channel)
    pos = r.integers(-400, 401, (T, D)).astype(np.float64)
    if overflow:
        bias[OVERFLOW_CH] = 7e4
    # Conv2d(C, D, 2, stride 2): out[b, d, gh, gw] = bias[d] + sum_{c, pi, qi} weight[d, c, pi, qi] z[b, c, 2 gh + pi, 2 gw + qi]; flatten(2).transpose(1, 2); + pos
    wt4 = w.reshape(D, C, 2, 2)
    zp = z.reshape(B, C, g, 2, g, 2)                              # [b, c, gh, pi, gw, qi]
    conv = np.einsum("dcpq,bchpwq->bhwd", wt4, zp)
    mag = np.einsum("dcpq,bchpwq->bhwd", np.abs(wt4), np.abs(zp))
    y = (conv + bias).reshape(B, T, D) + pos[None]
    delta = (K + 2) * U * ((mag + np.abs(bias)).reshape(B, T, D) + np.abs(pos)[None])
    return _ro(dict(C=C, g=g, B=B, D=D, K=K, T=T, rows=B * T, z=z.astype(F), w=w.astype(F), bias=bias.astype(F), pos=pos.astype(F),
                    y=y.reshape(B * T, D), delta=delta.reshape(B * T, D), overflow=overflow, name=f"C{C}-g{g}-B{B}-D{D}{'-overflow' if overflow else ''}"))


PATCH_MUTANTS = ("taps_exchanged", "pos_row_from_block", "tail_writes_neighbour", "bias_dropped", "clamp_not_counted", "transpose_skipped")


def transpose_restated(w):
    """k_transpose_f32: dst[k * N + n] = src[n * K + k], one element per thread"""
    N, K = w.shape
    i = np.arange(N * K)
    n, k = i // K, i % K
    dst = np.empty(N * K, F)
    dst[k * N + n] = w.ravel()[i]
    return dst.reshape(K, N)


def patch_restated(c, half, guard, mutant=None):
    """k_patch_embed<half, guard> in numpy float32, in its own order: the staged patch values (token clamped to the last row), acc = bias, acc += w * v for k ascending
    (product and sum rounded apart), + pos, the guard, the cast.  Returns (x [rows + 2][D] between one canary row before and one after -- NaN (fp32) / 0x7e00 (half
    bits) --, slot [max_bits, count] or None)."""
    C, g, D, K, T, rows = c["C"], c["g"], c["D"], c["K"], c["T"], c["rows"]
    S = 2 * g
    Wt = transpose_restated(c["w"]) if mutant != "transpose_skipped" else c["w"].reshape(K, D)
    z, bias, pos = c["z"], c["bias"], c["pos"]
    out = np.full((rows + 2 + PE_TOK, D), np.nan, F)            # (room for the mutant that writes past the end)
    mx, cnt = 0, 0
    for row0 in range(0, rows, PE_TOK):
        sp = np.empty((PE_TOK, K), F)
        for tk in range(PE_TOK):
            row = min(row0 + tk, rows - 1)
            t, b = row % T, row // T
            gh, gw = t // g, t % g
            for k in range(K):
                ch, pi, qi = k >> 2, (k >> 1) & 1, k & 1
                if mutant == "taps_exchanged":
                    pi, qi = qi, pi
                sp[tk, k] = z[b, ch, gh * 2 + pi, gw * 2 + qi]
        acc = np.tile(bias if mutant != "bias_dropped" else np.zeros(D, F), (PE_TOK, 1)).astype(F)
        for k in range(K):
            acc = (acc + (Wt[k][None, :] * sp[:, k:k + 1]).astype(F)).astype(F)
        for tk in range(PE_TOK):
            row = row0 + tk
            if row >= rows and mutant != "tail_writes_neighbour":
                continue
            pr = row % T if mutant != "pos_row_from_block" else min(row0 % T + tk, T - 1)     # mutant: the block's first token plus tk, never wrapped at a sample's end
            out[1 + row] = (acc[tk] + pos[pr]).astype(F)
    live = out[1:1 + rows]
    slot = None
    if guard:
        bits = live.view(np.uint32) & 0x7fffffff
        slot = [int(bits.max()), 0]
        if half:
            over = bits > 0x477fe000
            slot[1] = 0 if mutant == "clamp_not_counted" else int(over.sum())
            live[...] = np.where(np.isnan(live), live, np.clip(live, -HALF_MAX, HALF_MAX))
    out = out[:rows + 2]                                        # (the tail mutant's first stray row is the canary row after the last)
    if not half:
        return out, slot
    with np.errstate(over="ignore"):
        hb = out.astype(np.float16).view(np.uint16)
    hb[np.isnan(out)] = 0x7e00
    return hb, slot


def check_patch(c, half, x, wt=None, slot=None, plain=None):
    """x: the [rows + 2][D] buffer a call wrote into (fp32 values, or half bits), canary rows included.  wt: the transpose scratch [K * D + 2] between two NaN canaries.
    slot: the guard's two words after a guarded call; plain: the unguarded call's buffer, whose bytes a guarded in-range call must reproduce.
    Returns (list of failures as strings, worst ratio)."""
    rows, D, y, delta = c["rows"], c["D"], c["y"], c["delta"]
    fails = []
    body = x[1:-1]
    if half:
        hx = np.asarray(x, np.uint16)
        if not (np.all(hx[0] == 0x7e00) and np.all(hx[-1] == 0x7e00)): fails.append("canary row")
        k = np.asarray(body, np.uint16).view(np.float16).astype(np.float64)
    else:
        if not (np.all(np.isnan(x[0])) and np.all(np.isnan(x[-1]))): fails.append("canary row")
        k = np.asarray(body, np.float64)
    guarded = slot is not None
    yy, dd = y.copy(), delta.copy()
    if c["overflow"] and half:                                      # the documented behaviour beyond the half range: unguarded IEEE inf, guarded +-65,504 and counted
        col = k[:, OVERFLOW_CH]
        if not np.all(col == (HALF_MAX if guarded else np.inf)): fails.append("overflow channel")
        yy[:, OVERFLOW_CH], dd[:, OVERFLOW_CH], k = 0.0, 0.0, k.copy()
        k[:, OVERFLOW_CH] = 0.0
    bad, ratio = check_interval(yy, dd, k, "f16" if half else "f32")
    if bad: fails.append(f"{len(bad)} elements outside the radius, first at row {bad[0] // D} column {bad[0] % D}")
    if wt is not None:
        if not (np.isnan(wt[0]) and np.isnan(wt[-1])): fails.append("transpose canary")
        if not np.array_equal(np.asarray(wt[1:-1], F).view(np.uint32), np.ascontiguousarray(c["w"].T).ravel().view(np.uint32)): fails.append("transpose bytes")
    if guarded:
        want_max = int(np.abs(y).max().astype(F).view(np.uint32))   # (y is an exact integer below 2^24: the fp32 value before rounding)
        want_cnt = rows if (c["overflow"] and half) else 0
        if int(slot[0]) != want_max: fails.append(f"guard maximum {int(slot[0]):#x} != {want_max:#x}")
        if int(slot[1]) != want_cnt: fails.append(f"guard count {int(slot[1])} != {want_cnt}")
        if plain is not None and not c["overflow"] and not np.array_equal(np.asarray(x).view(np.uint8), np.asarray(plain).view(np.uint8)): fails.append("guarded bytes != unguarded bytes")
    return fails, ratio


# ---- k_unpatchify -----------------------------------------------------------------------------------------------------------------------------------------------

UNPATCH_OC = (8, 16, 3)
UNPATCH_G = (1, 3, 16)
UNPATCH_N = 2


@functools.lru_cache(maxsize=None)
def unpatch_case(OC, g):
    """tokens that hold their own flat index (exact in fp32: at most 2 * 256 * 64 of them); the reference is models.py:222-235"""
    N, p = UNPATCH_N, 2
    tok = np.arange(N * g * g * p * p * OC, dtype=np.float64).reshape(N, g * g, p * p * OC)
    x = tok.reshape(N, g, g, p, p, OC)
    imgs = np.einsum("nhwpqc->nchpwq", x).reshape(N, OC, g * p, g * p)
    return _ro(dict(OC=OC, g=g, N=N, tok=tok.astype(F), out=np.ascontiguousarray(imgs).astype(F)))


def unpatch_restated(c, mutant=None):
    """k_unpatchify's index arithmetic, one output element per thread.  mutant `c_and_taps_swapped`: the token's columns read as [c][pi][qi]"""
    OC, g, N = c["OC"], c["g"], c["N"]
    S = 2 * g
    i = np.arange(N * OC * S * S)
    xw, yh, ch, n = i % S, (i // S) % S, (i // (S * S)) % OC, i // (S * S * OC)
    col = ((yh & 1) * 2 + (xw & 1)) * OC + ch if mutant is None else ch * 4 + (yh & 1) * 2 + (xw & 1)
    return c["tok"].reshape(-1, 4 * OC)[n * g * g + (yh >> 1) * g + (xw >> 1), col].reshape(N, OC, S, S)


# ---- k_f32_to_bf16 ----------------------------------------------------------------------------------------------------------------------------------------------

def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


# ties in both directions (0x3f808000 = 1 + 2^-8 -> 1.0, even; 0x3f818000 = 1 + 3 * 2^-8 -> 1 + 2^-6), just off a tie, -0.0, bf16 sub-normals (0x00010000 the
# smallest; 0x00008000 half of it: a tie to zero; 0x00018000 a tie to 2; 0x00008001 just above), the largest finite fp32 (-> inf), the largest finite bf16, +-inf,
# NaNs (quiet, signalling, negative, one whose payload would carry into the exponent if it were rounded like a number)
SPECIAL_F32 = _f32([0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f808001, 0x3f807fff, 0x80000000, 0x00000000,
                    0x00010000, 0x00008000, 0x00018000, 0x00008001, 0x80018000, 0x007f8000, 0x7f7fffff, 0xff7fffff, 0x7f7f0000, 0x7f7f8000, 0x7f800000, 0xff800000,
                    0x7fc00000, 0x7f800001, 0xffc01234, 0x7fffffff])
CAST_N = (1, 255, 256, 1000)            # less than a block, one short of it, exactly one, several with a ragged last


@functools.lru_cache(maxsize=None)
def cast_case(n):
    r = np.random.default_rng(n)
    x = (r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n)).astype(F)
    m = min(n, len(SPECIAL_F32))
    x[:m] = SPECIAL_F32[:m] if n > 1 else SPECIAL_F32[1:2]
    return _ro(dict(n=n, x=x, bits=bf16_expected_bits(x), nan=np.isnan(x)))


# ---- k_vae_images / k_vae_latents / k_vae_quant -------------------------------------------------------------------------------------------------------------------

VAE_B = 2
IMAGES_R = (1, 6, 17)
LATENTS_R = (1, 5, 8)
LATENTS_C = (1, 4, 16, 64)              # 64: no spare channel
QUANT_N = (2, 8, 32, 64)
QUANT_HW = (1, 63, 64)


@functools.lru_cache(maxsize=None)
def images_case(R_):
    """img fp32 [B][3][R][R] with SPECIAL_F32 spread over the interior (as many as fit); expected bf16 bits [B][R+2][R+2][64]: +0 on the border and in channels >= 3"""
    r = np.random.default_rng(50 + R_)
    img = r.uniform(-1, 1, (VAE_B, 3, R_, R_)).astype(F)
    flat = img.reshape(-1)
    idx = r.permutation(flat.size)[:len(SPECIAL_F32)]
    flat[idx] = SPECIAL_F32[:len(idx)]
    if R_ == 1:
        flat[0] = -0.0                                           # the interior -0.0 must be there at every size
    exp = np.zeros((VAE_B, R_ + 2, R_ + 2, 64), np.uint16)
    exp[:, 1:-1, 1:-1, :3] = bf16_expected_bits(img).transpose(0, 2, 3, 1)
    nan = np.zeros(exp.shape, bool)
    nan[:, 1:-1, 1:-1, :3] = np.isnan(img).transpose(0, 2, 3, 1)
    assert np.any(img.view(np.uint32) == 0x80000000)
    return _ro(dict(R=R_, img=img, bits=exp, nan=nan))


def images_restated(c, mutant=None):
    R_ = c["R"]
    out = np.full((VAE_B, R_ + 2, R_ + 2, 64), 0x8000 if mutant == "border_minus_zero" else 0, np.uint16)
    out[:, 1:-1, 1:-1, :] = 0
    out[:, 1:-1, 1:-1, :3] = f32_to_bf16_bits(c["img"], truncate=mutant == "bf16_truncated").reshape(c["img"].shape).transpose(0, 2, 3, 1)
    return out


def _conv1x1(W, bias, v):
    """fp64 b + sum_k W[c][k] v[b][k][p], the sum of absolute terms with it, and the IEEE sign of an all-zero result (terms added one by one: -0 + -0 = -0)"""
    W, bias, v = W.astype(np.float64), bias.astype(np.float64), v.astype(np.float64)
    y = np.broadcast_to(bias[None, :, None], (v.shape[0], W.shape[0], v.shape[2])).copy()
    mag = np.abs(y)
    for k in range(W.shape[1]):
        t = W[None, :, k, None] * v[:, None, k, :]
        y = y + t
        mag = mag + np.abs(t)
    return y, mag


@functools.lru_cache(maxsize=None)
def latents_case(C, r_):
    """z [B][C][r][r], W [C][C], bias [C] ~ N(0, 1).  C >= 4: channel C - 1 has bias -0.0 and a row of -0.0 weights, and z >= 0 at pixel (0, 0) of every sample, so that the
    interior element (b, 1, 1, C - 1) is -0.0 and must keep its sign; every other pixel of that channel sees negative z as well and is +0 or -0 as IEEE has it."""
    r = np.random.default_rng(900 + 10 * C + r_)
    z = r.standard_normal((VAE_B, C, r_, r_)).astype(F)
    W = r.standard_normal((C, C)).astype(F)
    bias = r.standard_normal(C).astype(F)
    if C >= 4:
        W[C - 1] = -0.0
        bias[C - 1] = -0.0
        z[:, :, 0, 0] = np.abs(z[:, :, 0, 0])
    y, mag = _conv1x1(W, bias, z.reshape(VAE_B, C, r_ * r_))
    full = np.zeros((VAE_B, r_ + 2, r_ + 2, 64))
    delta = np.zeros_like(full)
    full[:, 1:-1, 1:-1, :C] = y.reshape(VAE_B, C, r_, r_).transpose(0, 2, 3, 1)
    delta[:, 1:-1, 1:-1, :C] = (C + 1) * U * mag.reshape(VAE_B, C, r_, r_).transpose(0, 2, 3, 1)
    interior = np.zeros(full.shape, bool)
    interior[:, 1:-1, 1:-1, :C] = True
    return _ro(dict(C=C, r=r_, z=z, W=W, bias=bias, y=full, delta=delta, interior=interior))


def latents_restated(c, mutant=None):
    C, r_ = c["C"], c["r"]
    W = c["W"].T if mutant == "W_transposed" else c["W"]
    v = c["z"].reshape(VAE_B, C, r_ * r_)
    acc = np.broadcast_to(c["bias"][None, :, None], (VAE_B, C, r_ * r_)).astype(F)
    for k in range(C):
        acc = (acc + (W[None, :, k, None] * v[:, None, k, :]).astype(F)).astype(F)
    out = np.full((VAE_B, r_ + 2, r_ + 2, 64), 0x8000 if mutant == "border_minus_zero" else 0, np.uint16)
    out[:, 1:-1, 1:-1, :] = 0
    out[:, 1:-1, 1:-1, :C] = f32_to_bf16_bits(acc, truncate=mutant == "bf16_truncated").reshape(VAE_B, C, r_, r_).transpose(0, 2, 3, 1)
    return out


def check_latents(c, bits):
    """outside the interior's first C channels +0 BITS; inside, the interval; the -0.0 element's sign.  Returns (failures, worst ratio)."""
    bits = np.asarray(bits, np.uint16).reshape(c["y"].shape)
    fails = []
    if np.any(bits[~c["interior"]] != 0): fails.append("border or spare channel not +0")
    bad, ratio = check_interval(c["y"][c["interior"]], c["delta"][c["interior"]], bf16_bits_to_f64(bits[c["interior"]]), "bf16")
    if bad: fails.append(f"{len(bad)} interior elements outside the radius")
    if c["C"] >= 4 and np.any(bits[:, 1, 1, c["C"] - 1] != 0x8000): fails.append("interior -0.0 lost its sign")
    return fails, ratio


@functools.lru_cache(maxsize=None)
def quant_case(N, hw):
    r = np.random.default_rng(7000 + 100 * N + hw)
    m = (r.standard_normal((VAE_B, N, hw)) * 3.0).astype(F)
    W = r.standard_normal((N, N)).astype(F)
    bias = r.standard_normal(N).astype(F)
    y, mag = _conv1x1(W, bias, m)
    return _ro(dict(N=N, hw=hw, m=m, W=W, bias=bias, y=y, delta=(N + 1) * U * mag))


def quant_restated(c, mutant=None):
    W = c["W"].T if mutant == "W_transposed" else c["W"]
    acc = np.broadcast_to(c["bias"][None, :, None], c["m"].shape).astype(F)
    for k in range(c["N"]):
        acc = (acc + (W[None, :, k, None] * c["m"][:, None, k, :]).astype(F)).astype(F)
    return acc


# ---- k_dit_time_freq --------------------------------------------------------------------------------------------------------------------------------------------

TIME_STEPS = (0.0, 1e-3, 1.0, 3.0, 500.0, 999.0, 1000.0)
TIME_B = (3, 7, 4100)                   # 4100: 4,101 blocks -- the DiT plan used to launch this kernel under a cap of 4,096 blocks
EXP_ULPS, TRIG_ULPS, VEXP_ULPS = 3.0, 4.0, 1.0              # the starting bounds of the module docstring
TIME_MEASURED, SILU_MEASURED = 0.0, 0.0                      # MI355X: the worst unexplained part, in units of the allowance (module docstring)


@functools.lru_cache(maxsize=None)
def time_case(B, dev=True):
    """t = three of TIME_STEPS (B = 3), else all of them in turn; y fp64 [B][256] = [cos | sin]; delta = |a| rho + the device allowance (dev = False: the analytic part
    alone, for measuring)"""
    t = np.array((TIME_STEPS[3], TIME_STEPS[6], TIME_STEPS[1]) if B == 3 else [TIME_STEPS[i % 7] for i in range(B)], F)
    h = np.arange(128, dtype=np.float64)
    e = -LN1E4 * h / 128.0
    a = t.astype(np.float64)[:, None] * np.exp(e)[None, :]
    y = np.concatenate([np.cos(a), np.sin(a)], axis=1)
    rho = (2.0 * np.abs(e) + 1.0) * U
    d = np.abs(a) * rho[None, :] + (np.abs(a) * EXP_ULPS * 2 * U + TRIG_ULPS * 2 * U if dev else 0.0)
    return _ro(dict(B=B, t=t, y=y, delta=np.concatenate([d, d], axis=1)))


def time_restated(c, mutant=None):
    t = c["t"]
    i = np.arange(c["B"] * 256)
    b, j = i >> 8, i & 255
    h = (j & 127).astype(F)
    with np.errstate(over="ignore"):
        f = np.exp((F(-np.log(1e3) if mutant == "max_period_1e3" else -9.210340371976184) * h) / F(127.0 if mutant == "h_over_127" else 128.0)).astype(F)
    a = (t[b] * f).astype(F)
    first = (j < 128) if mutant != "sin_cos_order" else (j >= 128)
    v = np.where(first, np.cos(a), np.sin(a)).astype(F)
    return f32_to_bf16_bits(v).reshape(c["B"], 256), v.reshape(c["B"], 256)


# ---- k_silu_bf16 / k_dit_cond -----------------------------------------------------------------------------------------------------------------------------------

def silu_reference(s, pre_rounded, dev=True):
    """fp64 SiLU(s) and its radius (module docstring); pre_rounded: s itself was rounded to fp32 first (k_dit_cond's sum)"""
    s = np.asarray(s, np.float64)
    with np.errstate(over="ignore"):
        E = np.exp(-s)
        y = s / (1.0 + E)
        w = np.where(np.isinf(E), 1.0, E / (1.0 + E))
    rel = U * (2.0 + w * (2.0 * np.abs(s) + (VEXP_ULPS * 2 if dev else 0.0)))
    delta = np.abs(y) * rel + FLOOR + (1.1 * U * np.abs(s) if pre_rounded else 0.0)
    return y, delta


def silu_restated(s):
    """silu_f in float32: v / (1 + exp2(fl(-v log2 e)))"""
    s = np.asarray(s, F)
    with np.errstate(over="ignore"):
        E = np.exp2((-s * F(1.4426950408889634)).astype(F)).astype(F)
        return (s / (F(1.0) + E)).astype(F)


SILU_N = (1, 256, 777)


@functools.lru_cache(maxsize=None)
def silu_case(n, dev=True):
    r = np.random.default_rng(300 + n)
    x = r.standard_normal(n).astype(F)
    sp = np.array([100.0, -100.0, 0.0, -0.0, 88.0, -88.0, 20.0, -20.0, 1e-30, -5.5], F)
    x[:min(n, len(sp))] = sp[:min(n, len(sp))]
    y, delta = silu_reference(x, False, dev)
    return _ro(dict(n=n, x=x, y=y, delta=delta))


COND_D = (64, 1152)                     # four samples per 256-thread block; sample boundaries inside blocks
COND_B = 3
COND_LARGE = (1152, 920)                # D, B: 4,140 blocks -- the DiT plan used to launch this kernel under a cap of 4,096 blocks: B >= 911 at D = 1152
COND_CLASSES = 11                       # table rows 0 .. 10; row 10 is the null class (DiT: 1000 of 1001)
COND_LABELS = (0, 4, 10)


@functools.lru_cache(maxsize=None)
def cond_case(D, B=COND_B, dev=True):
    """c0 [B][D] and the three selected table rows span +-100, 0 and N(0, 1); every table row the labels do not select is NaN; sample b has label COND_LABELS[b % 3]"""
    r = np.random.default_rng(400 + D + B)
    c0 = r.standard_normal((B, D)).astype(F)
    c0[0, ::5] = 100.0; c0[1, 1::5] = -100.0; c0[2, 2::7] = 0.0
    table = np.full((COND_CLASSES, D), np.nan, F)
    for lab in COND_LABELS:
        table[lab] = r.standard_normal(D)
    table[0, ::3] = 0.0
    table[10, 1::4] = -100.0; table[10, ::9] = 100.0
    y32 = np.array([COND_LABELS[b % 3] for b in range(B)], np.int32)
    s = c0.astype(np.float64) + table[y32].astype(np.float64)
    y, delta = silu_reference(s, True, dev)
    return _ro(dict(D=D, B=B, c0=c0, table=table, labels=y32, y=y, delta=delta))


def cond_restated(c, mutant=None):
    lab = c["labels"].copy()
    if mutant == "null_row_off_by_one":
        lab[lab == COND_CLASSES - 1] -= 1
    return silu_restated((c["c0"] + c["table"][lab]).astype(F))
