"""Inputs, fp64 references and comparators for the row kernels tested alone (tests/test_row_kernels_host.py on the CPU, tests/test_gpu_row_kernels.py on the GPU):
LayerNorm-modulate (k_ln_modulate, k_ln_modulate_v4, k_ln_modulate_h8: csrc/transformer_rows.h) to bf16 (their RowsBf16 instances) and to fp8 e4m3 with a scale per
row (their RowsFp8 instances), the row quantiser k_pack_fp8_rows, and the three row softmaxes (k_softmax_rows, k_softmax_rows_1k, k_softmax_rows_wide).  numpy only.

u = 2^-24 is the unit roundoff of fp32 (every kernel keeps its statistics and its arithmetic in fp32).

LayerNorm-modulate.  Per element, in fp64 from the exact input values (the half stream's inputs are the fp16 values):
    n = (x - mean) / sigma,  sigma = sqrt(var + float32(1e-6)),  var the BIASED variance,  y = n (1 + sc) + sh.
Error radius of a correct fp32 kernel:
    delta   = delta_n |1 + sc| + 4u (|n (1 + sc)| + |sh|),
    delta_n = u (32 mean|x_row| / sigma + 24 |n|).
Derivation, from the kernels' code.  (a) The mean: a lane adds at most 24 values (D <= 1536, 64 lanes) and the butterfly adds 6 levels, so the longest fp32
addition chain has under 32 links and |mean_k - mean| <= 32u mean|x| (each link's error is at most u times a partial sum of absolute values, and the mean of those
bounds is 32u mean|x_row|, first order).  Dividing by sigma gives the first term of delta_n: every element of the row is shifted by that much.  (b) x - mean_k is one
rounding: u |x - mean| / sigma = u |n|.  (c) The sum of squares has only positive terms, so its relative error is at most the chain length plus the two roundings of
each square, (32 + 2)u, halved by the square root: 17u; the division by D, the addition of epsilon, the square root and the reciprocal add u each, 21u; the product
with rstd one more, 22u; with (b) 23u |n| -- 24 |n| with the second-order term that the mean's error leaves in the squares (sum (x - mean_k)^2 = sum (x - mean)^2 + D
(mean_k - mean)^2, the cross term vanishes).  (d) 1 + sc, the product with it, the addition of sh: 2u |n (1 + sc)| + u |y|, and u |y| <= u (|n (1 + sc)| + |sh|);
4u covers a kernel that contracts the last product and the addition into one fma as well as one that does not.
A numpy-float32 restatement of the scalar form stays within 0.25 delta over D in {64, 256, 1152, 1536} and every row family below
(test_row_kernels_host.py::test_restated_ln_forms_pass prints the figure).  If a kernel exceeds delta that is a finding to explain: the radius changes only with a
written derivation of the missing term.

Comparators.  bf16: the kernel's value must lie in [rne_bf16(y - delta), rne_bf16(y + delta)] -- every element, no mask.  fp8: see check_fp8.  softmax: see
check_softmax."""
import functools

import numpy as np

U = 2.0 ** -24
EPS32 = float(np.float32(1e-6))
B, RPS = 3, 5                   # samples, rows per sample: 15 rows -- a last block with three live waves, two sample boundaries inside a block
ROWS = B * RPS
NMOD = 6                        # mod_ld = 6 D (+ 1), shift at D, scale at 2 D: the engines' nmod layout
LN_D_VECTOR = (256, 1152, 1536)
LN_D_SCALAR = (64, 128, 384, 1536 - 128)
LAYOUTS = ("aligned", "moved_one_float", "odd_mod_ld")
# one family per row, numbered as in ln_case below: 4 and 7 are the constant rows; sample 2 has sh = 0 (family 7 needs it), samples 0 and 1 a random one
FAMILIES = (1, 2, 3, 4, 5,   6, 1, 4, 5, 2,   7, 1, 6, 3, 7)
HALF_EXTRA_ROW = 6              # half stream: this row holds fp16 sub-normals and +-60000 instead (family "H")


# ---- number formats -----------------------------------------------------------------------------------------------------------------------------------------------

def rne_bf16(v):
    """fp64 -> the nearest bf16 value (ties to even), returned as fp64; sub-normals kept, beyond the largest finite value +-inf"""
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    _, e = np.frexp(a)                                          # a = m 2^e, m in [0.5, 1)
    q = np.exp2(np.maximum(e - 1, -126).astype(np.float64) - 7)     # the spacing of bf16 at a (8 significant bits)
    r = np.rint(a / q) * q                                      # np.rint: ties to even; a / q is exact (a power of two)
    r = np.where(r > (2.0 - 2.0 ** -7) * 2.0 ** 127, np.inf, r)
    return np.copysign(r, v)


def bf16_bits_to_f64(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def f32_to_bf16_bits(v):
    """fp32 -> bf16 bits, round to nearest even (what `(bf16)float` compiles to); finite inputs"""
    w = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((w + 0x7fff + ((w >> 16) & 1)) >> 16).astype(np.uint16)


def half_ulp_bf16(v):
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))
    return np.exp2(np.maximum(e - 1, -126).astype(np.float64) - 8)


def _e4m3_table():
    t = np.empty(256, np.float64)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        v = m * 2.0 ** -9 if e == 0 else (np.nan if (e == 15 and m == 7) else 2.0 ** (e - 7) * (1 + m / 8))
        t[b] = -v if b & 0x80 else v
    return t


E4M3 = _e4m3_table()            # e4m3fn by formula: bias 7, sub-normals m 2^-9, no infinity, 0x7f / 0xff NaN, largest finite 448 = 0x7e
_E4M3_POS = E4M3[:0x7f]         # 0 .. 448, increasing with the byte


def e4m3_ulp(v):
    """2^-9 below 2^-6, 2^(floor(log2 |v|) - 3) above (|v| capped at 448: the format ends there)"""
    a = np.minimum(np.abs(np.asarray(v, np.float64)), 448.0)
    _, e = np.frexp(np.maximum(a, 2.0 ** -6))
    return np.exp2((e - 1).astype(np.float64) - 3)


def f32_to_e4m3(v, truncate=False, saturate_first=True):
    """fp32 -> e4m3fn bytes, round to nearest even (truncate: toward zero -- a mutant).  saturate_first: clamp to +-448 before the conversion, as the kernels do;
    without it (a mutant) the conversion is the pessimistic model of a non-saturating convert: any magnitude above 448 is out of range and encodes NaN."""
    v = np.asarray(v, np.float32).astype(np.float64)
    a = np.abs(v)
    over = a > 448.0
    a = np.minimum(a, 448.0)
    hi = np.clip(np.searchsorted(_E4M3_POS, a, side="left"), 1, 0x7e)
    lo = hi - 1
    dl, dh = a - _E4M3_POS[lo], _E4M3_POS[hi] - a
    up = (dh == 0) if truncate else ((dh < dl) | ((dh == dl) & (hi % 2 == 0)))
    b = np.where(up, hi, lo).astype(np.uint8)
    if not saturate_first:
        b = np.where(over, 0x7f, b).astype(np.uint8)
    return (b | np.where(np.signbit(v), 0x80, 0).astype(np.uint8)).astype(np.uint8)


# ---- LayerNorm-modulate: cases ----------------------------------------------------------------------------------------------------------------------------------

def expected_form(D, half, layout):
    """what launch_ln_modulate must choose (either output policy): 0 scalar, 1 four-column, 2 eight-column"""
    if layout != "aligned" or D not in LN_D_VECTOR:
        return 0
    return 2 if (half and D == 1536) else 1


def ln_case_ids(fp8):
    ids = [(D, half, lay) for half in (False, True) for D in LN_D_VECTOR for lay in LAYOUTS]
    ids += [(D, half, "aligned") for half in (False, True) for D in LN_D_SCALAR if not (fp8 and D % 128)]
    return ids


@functools.lru_cache(maxsize=None)
def ln_case(D, half, layout):
    """one call: x [ROWS][D] (fp32, or fp16 when half), mod [B][mod_ld] fp32 with shift at `shift_off` and scale at `scale_off` floats (every other float NaN), and
    the fp64 reference y with its radius delta.  Arrays are read-only: the tests share them."""
    r = np.random.default_rng(1000 * D + 10 * LAYOUTS.index(layout) + int(half))
    x = np.empty((ROWS, D), np.float64)
    for i, f in enumerate(FAMILIES):
        g = r.standard_normal(D)
        if f == 1: x[i] = g
        elif f == 2: x[i] = 100.0 + 0.01 * g
        elif f == 3: x[i] = 1e-3 * g                             # the epsilon decides the result
        elif f in (4, 7): x[i] = 0.5                             # sums exact: the output is the shift, exactly
        elif f == 5: x[i] = g; x[i, D - 3] = 1e4                 # column D - 3: in the 128-column tail chunk of 1152
        elif f == 6: x[i] = 300.0 * g
    fam = list(FAMILIES)
    if half:
        h = r.standard_normal(D) * 3e-6                          # fp16 sub-normals (below 6.1e-5) ...
        h[::7] = 60000.0 * np.where(r.random(len(h[::7])) < 0.5, -1.0, 1.0)      # ... and +-60000
        x[HALF_EXTRA_ROW] = h
        fam[HALF_EXTRA_ROW] = "H"
    xs = x.astype(np.float16) if half else x.astype(np.float32)
    mod_ld = NMOD * D + (1 if layout == "odd_mod_ld" else 0)
    shift_off, scale_off = (D + 1, 2 * D + 1) if layout == "moved_one_float" else (D, 2 * D)
    mod = np.full((B, mod_ld), np.nan, np.float32)
    sc = r.uniform(-1.5, 1.5, (B, D)).astype(np.float32)
    sh = (2.0 * r.standard_normal((B, D))).astype(np.float32)
    sh[2] = 0.0
    mod[:, shift_off:shift_off + D] = sh
    mod[:, scale_off:scale_off + D] = sc
    y, delta = ln_reference(xs, sh, sc, RPS)
    c = dict(D=D, half=half, layout=layout, x=xs, mod=mod, mod_ld=mod_ld, shift_off=shift_off, scale_off=scale_off, shift=sh, scale=sc, families=tuple(fam),
             y=y, delta=delta, form=expected_form(D, half, layout), name=f"D{D}-{'f16' if half else 'f32'}-{layout}")
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def ln_reference(x, shift, scale, rps):
    """fp64 y [rows][D] and the radius delta (module docstring); x fp32 or fp16 [rows][D], shift / scale fp32 [B][D]"""
    x = x.astype(np.float64)
    b = np.arange(x.shape[0]) // rps
    sh, sc = shift.astype(np.float64)[b], scale.astype(np.float64)[b]
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    sigma = np.sqrt(var + EPS32)
    n = (x - mean) / sigma
    y = n * (1.0 + sc) + sh
    delta_n = U * (32.0 * np.abs(x).mean(axis=1, keepdims=True) / sigma + 24.0 * np.abs(n))
    delta = delta_n * np.abs(1.0 + sc) + 4.0 * U * (np.abs(n * (1.0 + sc)) + np.abs(sh))
    return y, delta


def exact_rows(c):
    """rows whose result is the shift exactly (families 4 and 7): every sum over a constant 0.5 is exact in fp32, x - mean = 0"""
    return [i for i, f in enumerate(c["families"]) if f in (4, 7)]


# ---- LayerNorm-modulate: numpy-float32 restatements of the kernel forms ---------------------------------------------------------------------------------------

F = np.float32


def _butterfly(a, op=np.add):
    """the __shfl_xor reduction over the 64 lanes (axis 1): o = 32, 16, ..., 1; every lane ends with the same value"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = op(a, a[:, lanes ^ o])
    return a[:, :1]


def _lane_sums(v, form, fp8, what):
    """per-lane partial sums of v [rows][D] (fp32) in the summation order of the form: [rows][64].  what: "sum" or "squares" (the scalar fp8 form orders them apart)"""
    rows, D = v.shape
    s = np.zeros((rows, 64), F)
    if form == 0 and not fp8:                                   # k_ln_modulate: lane l owns columns l + 64 i, added one by one
        for i in range(D // 64):
            s = s + v[:, 64 * i:64 * i + 64]
    elif form == 0:                                             # k_ln_modulate<RowsFp8>: columns 2 l, 2 l + 1 of every 128; the sum adds the pair first, the squares one by one
        for i in range(D // 128):
            p = v[:, 128 * i:128 * i + 128].reshape(rows, 64, 2)
            if what == "sum": s = s + (p[:, :, 0] + p[:, :, 1])
            else: s = (s + p[:, :, 0]) + p[:, :, 1]
    elif form == 1:                                             # *_v4: four consecutive columns per 256-column chunk, (x + y) + (z + w); the partial chunk: lanes < REM / 4
        for i in range(-(-D // 256)):
            w = v[:, 256 * i:256 * i + 256]
            if w.shape[1] < 256:
                w = np.concatenate([w, np.zeros((rows, 256 - w.shape[1]), F)], axis=1)
            p = w.reshape(rows, 64, 4)
            s = s + ((p[:, :, 0] + p[:, :, 1]) + (p[:, :, 2] + p[:, :, 3]))
    else:                                                       # *_h8: eight consecutive columns per 512-column chunk, a balanced tree
        for i in range(D // 512):
            p = v[:, 512 * i:512 * i + 512].reshape(rows, 64, 8)
            s = s + (((p[:, :, 0] + p[:, :, 1]) + (p[:, :, 2] + p[:, :, 3])) + ((p[:, :, 4] + p[:, :, 5]) + (p[:, :, 6] + p[:, :, 7])))
    return s


LN_MUTANTS = ("eps_1e-5", "var_over_D-1", "stats_without_tail", "tail_rotated_by_4", "shift_scale_swapped", "sample_index_row+1")
FP8_MUTANTS = ("e4m3_truncated", "no_clamp", "amax_before_modulation")


def ln_restated(c, form, fp8, mutant=None):
    """The modulated rows in fp32 [rows][D] as the kernel form computes them (unfused multiply and add), and for the fp8 mutant `amax_before_modulation` the rows the
    row maximum is taken from.  form: 0 / 1 / 2.  mutant: one of LN_MUTANTS (or None)."""
    D, REM = c["D"], c["D"] % 256
    x = c["x"].astype(F)
    rows = x.shape[0]
    ns = D - REM if mutant == "stats_without_tail" else D      # mutant: the partial chunk is left out of the statistics
    xs = x[:, :ns] if ns != D else x
    mean = _butterfly(_lane_sums(xs, form, fp8, "sum")) / F(ns)
    d = xs - mean
    q = _butterfly(_lane_sums(d * d, form, fp8, "squares")) / F(D - 1 if mutant == "var_over_D-1" else ns)
    rstd = F(1.0) / np.sqrt(q + F(1e-5 if mutant == "eps_1e-5" else 1e-6))
    b = (np.arange(rows) + (1 if mutant == "sample_index_row+1" else 0)) // RPS
    sh, sc = c["shift"], c["scale"]
    if mutant == "shift_scale_swapped":
        sh, sc = sc, sh
    if b.max() >= sh.shape[0]:                                  # (the off-by-one mutant reads a sample that does not exist: give it one)
        sh, sc = np.concatenate([sh, sh[:1]]), np.concatenate([sc, sc[:1]])
    n = (x - mean) * rstd
    if mutant == "tail_rotated_by_4":                           # mutant: the partial chunk's columns land four to the right
        n = np.concatenate([n[:, :D - REM], np.roll(n[:, D - REM:], 4, axis=1)], axis=1)
    return (n * (F(1.0) + sc[b]) + sh[b]).astype(F), n.astype(F)


def quant_restated(v, mutant=None, amax_from=None):
    """k_pack_fp8_rows / the tail of the k_ln_modulate*<..., RowsFp8> kernels on fp32 rows: scale = amax / 448 (1.0 for an all-zero row), bytes = e4m3(clamp(v * (1 / scale)))"""
    v = np.asarray(v, F)
    amax = np.abs(v if amax_from is None else amax_from).max(axis=1, keepdims=True).astype(F)
    qs = np.where(amax > 0, amax / F(448.0), F(1.0)).astype(F)
    t = (v * (F(1.0) / qs)).astype(F)
    q = f32_to_e4m3(t, truncate=mutant == "e4m3_truncated", saturate_first=mutant != "no_clamp")
    return q, qs[:, 0]


# ---- comparators ------------------------------------------------------------------------------------------------------------------------------------------------

def check_bf16(c, bits):
    """bits: uint16 [rows][D].  Returns (failing rows, worst (|k - y| - half a bf16 ulp) / delta): the second is a figure to print, the first decides."""
    k = bf16_bits_to_f64(bits)
    y, delta = c["y"], c["delta"]
    ok = (k >= rne_bf16(y - delta)) & (k <= rne_bf16(y + delta))            # (a NaN fails both)
    for i in exact_rows(c):                                                 # the output IS bf16(shift)
        ok[i] &= k[i] == bf16_bits_to_f64(f32_to_bf16_bits(c["shift"][i // RPS]))
    with np.errstate(invalid="ignore"):
        ratio = np.nanmax(np.maximum(np.abs(k - y) - half_ulp_bf16(k), 0.0) / delta)
    return sorted(set(np.nonzero(~ok.all(axis=1))[0].tolist())), float(ratio)


def check_fp8(y, delta, q, scale, exact=()):
    """y, delta fp64 [rows][K] (delta None: zero); q uint8 [rows][K]; scale fp32 [rows]: what a kernel wrote.  Rows in `exact` are checked with delta = 0.
    Per row, with amax = max |y|, delta_amax the radius of that element, s = the kernel's scale:
      * amax = 0: s = 1.0 and every byte 0;
      * |s - amax / 448| <= (delta_amax / amax + 4u) amax / 448 -- with delta = 0: s equal to float32(amax) / 448 up to 2u;
      * no byte 0x7f / 0xff; the byte of the largest element exactly 0x7e / 0xfe;
      * |decode(byte) - y / s| <= half an e4m3 ulp + delta / s, the ulp taken at the largest magnitude the kernel's scaled value can have, |y / s| + delta / s.
    Returns (failing rows, worst (|decode - y / s| - half ulp) / (delta / s) over the rows with delta > 0)."""
    y = np.asarray(y, np.float64)
    delta = np.zeros_like(y) if delta is None else np.array(delta, np.float64)
    delta[list(exact)] = 0.0
    s = np.asarray(scale, np.float32).astype(np.float64)
    bad, worst = [], 0.0
    for i in range(y.shape[0]):
        a = np.abs(y[i]); j = int(a.argmax()); amax = a[j]
        if amax == 0.0:
            if not (s[i] == 1.0 and not q[i].any()): bad.append(i)
            continue
        rel = delta[i, j] / amax + (4.0 * U if delta[i, j] > 0 else 2.0 * U)
        row_ok = np.isfinite(s[i]) and s[i] > 0 and abs(s[i] - amax / 448.0) <= rel * amax / 448.0
        row_ok = row_ok and not np.any((q[i] & 0x7f) == 0x7f) and (q[i, j] & 0x7f) == 0x7e and bool(q[i, j] & 0x80) == bool(y[i, j] < 0)
        if row_ok:
            t, slack = y[i] / s[i], delta[i] / s[i]
            err = np.abs(E4M3[q[i]] - t) - 0.5 * e4m3_ulp(np.abs(t) + slack)
            row_ok = bool(np.all(err <= slack))
            if slack.max() > 0:
                worst = max(worst, float(np.max(np.maximum(err, 0.0)[slack > 0] / slack[slack > 0])))
        if not row_ok: bad.append(i)
    return bad, worst


# ---- k_pack_fp8_rows ---------------------------------------------------------------------------------------------------------------------------------------------

PACK_K = (2, 130, 1152)
PACK_ROW_KINDS = ("normal", "zero", "negative_max")


@functools.lru_cache(maxsize=None)
def pack_case(K, kinds):
    """fp32 rows [len(kinds)][K]: `normal` N(0, 1) times 10^(row - 2), `zero` all zero, `negative_max` N(0, 1) whose largest magnitude is a negative entry"""
    r = np.random.default_rng(77 * K + len(kinds))
    w = np.empty((len(kinds), K), np.float32)
    for i, kind in enumerate(kinds):
        g = r.standard_normal(K) * 10.0 ** (i - 2)
        if kind == "zero": g[:] = 0.0
        if kind == "negative_max": g[r.integers(K)] = -1.5 * np.abs(g).max() - 1.0
        w[i] = g
    w.setflags(write=False)
    return w


def pack_cases():
    return [(K, kinds) for K in PACK_K for kinds in ((("normal",), ("zero",), ("negative_max",), ("normal", "zero", "normal", "negative_max", "normal")))]


# ---- softmax ----------------------------------------------------------------------------------------------------------------------------------------------------

SOFTMAX_T = {0: (16, 64, 100, 256), 1: (64, 576, 1024), 2: (64, 1088, 4096)}
SOFTMAX_FAMILIES = ("all_equal", "normal", "normal_x30", "dominant_first", "dominant_middle", "dominant_last", "two_equal_maxima")
FLOOR = 2.0 ** -126                                             # sub-normal results may be flushed


@functools.lru_cache(maxsize=None)
def softmax_rows(T, families):
    r = np.random.default_rng(31 * T + len(families))
    s = np.empty((len(families), T), np.float32)
    for i, f in enumerate(families):
        g = r.standard_normal(T)
        if f == "all_equal": g[:] = 3.25                         # 1 / T: exact when T is a power of two
        elif f == "normal_x30": g *= 30.0                        # the small probabilities underflow
        elif f.startswith("dominant"): g[{"first": 0, "middle": T // 2, "last": T - 1}[f.split("_")[1]]] = 80.0
        elif f == "two_equal_maxima": g[:] = -1e4; g[1] = g[T - 2] = 2.5
        s[i] = g
    s.setflags(write=False)
    return s


def softmax_cases():
    """(kind, T, families): seven rows with one family each, and every family as a one-row call"""
    return [(k, T, fams) for k in (0, 1, 2) for T in SOFTMAX_T[k] for fams in [SOFTMAX_FAMILIES] + [(f,) for f in SOFTMAX_FAMILIES]]


def softmax_reference(s):
    """fp64 p and the relative radius eps = u (16 + T / 64 + 4 |s - max|): the native exp2 path costs about 2u |s - max| + 3u (the product with log2 e is rounded to
    fp32 before the exponential: an absolute error of u |s - max| log2 e in the exponent, twice for the numerator and the terms of the sum), the sum chain T / 64 + 6
    links, the reciprocal and the product 2u"""
    s = s.astype(np.float64)
    d = s - s.max(axis=1, keepdims=True)
    e = np.exp(d)
    return e / e.sum(axis=1, keepdims=True), U * (16.0 + s.shape[1] / 64.0 + 4.0 * np.abs(d))


def check_softmax(s, families, bits):
    """bits uint16 [rows][T].  Accepts [rne_bf16(p (1 - eps) - floor), rne_bf16(p (1 + eps) + floor)], every element; an all-equal row of a power-of-two T must be
    bf16(1 / T) exactly.  Returns (failing rows, worst (|k - p| - half a bf16 ulp - floor) / (eps p))."""
    k = bf16_bits_to_f64(bits)
    p, eps = softmax_reference(s)
    ok = (k >= rne_bf16(p * (1 - eps) - FLOOR)) & (k <= rne_bf16(p * (1 + eps) + FLOOR))
    T = s.shape[1]
    for i, f in enumerate(families):
        if f == "all_equal" and T & (T - 1) == 0:
            ok[i] &= k[i] == 1.0 / T
    with np.errstate(invalid="ignore", divide="ignore"):
        m = p > 2.0 ** -100
        ratio = np.nanmax(np.where(m, np.maximum(np.abs(k - p) - half_ulp_bf16(k) - FLOOR, 0.0) / np.where(m, eps * p, 1.0), 0.0))
    return np.nonzero(~ok.all(axis=1))[0].tolist(), float(ratio)


def softmax_restated(s, kind, mutant=None):
    """numpy-float32 restatement of the three kernels: exp(x) as exp2(float32(x log2 e)), the per-lane sums in each kernel's order (they coincide: lane l adds columns
    l, l + 64, ... in turn), the butterfly, one reciprocal.  mutant: `no_max_subtraction` / `normalised_by_T`."""
    s = s.astype(F)
    rows, T = s.shape
    pad = -T % 64                                               # kind 0: the columns past T count as -inf / 0
    mx = np.zeros((rows, 1), F) if mutant == "no_max_subtraction" else s.max(axis=1, keepdims=True)
    with np.errstate(over="ignore"):
        e = np.exp2(((s - mx) * F(1.4426950408889634)).astype(F)).astype(F)
    ep = np.concatenate([e, np.zeros((rows, pad), F)], axis=1)
    lane = np.zeros((rows, 64), F)
    for i in range(ep.shape[1] // 64):
        lane = lane + ep[:, 64 * i:64 * i + 64]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):     # (the mutant without the max subtraction overflows: that is how it shows)
        tot = F(T) if mutant == "normalised_by_T" else _butterfly(lane)
        out = (e * (F(1.0) / tot)).astype(F)
    return f32_to_bf16_bits(np.nan_to_num(out, nan=0.0, posinf=3e38))
