"""Inputs, fp64 references, radii, comparators, numpy-float32 restatements and mutants for the GroupNorm, output-head and glue kernels of the NCSN++ / AutoencoderKL
engines tested alone: k_gn_stats, k_gn_finalize, k_gn_apply, k_time_embed, k_stem_im2col, k_pack_conv, k_pack_transpose, k_nhwc_to_nchw_f32 (csrc/ncsnpp_kernels.h),
k_gn_fold (csrc/vae_engine.inc) and k_head_conv (csrc/head_conv.h).  tests/test_gn_kernels_host.py runs them on the CPU, tests/test_gpu_gn_kernels.py on the GPU through
the natinf_debug_* entry points at the end of include/natinf_ncsnpp.h.  numpy only.

u = 2^-24, the unit roundoff of fp32.  Inputs are bf16 values and every reference is computed in fp64 from exactly those values.  A bf16 output k of a value y with
radius delta passes when rne_bf16(y - delta) <= k <= rne_bf16(y + delta); an fp32 output t with an interval [lo, hi] passes when lo <= t <= hi.  Every element is
compared, none is masked (a NaN fails both comparisons).  Where a figure `worst error / radius` is printed, the half bf16 ulp of the output's own rounding is not counted.

GroupNorm tables (k_gn_stats, ncsnpp_kernels.h:524-574; k_gn_finalize, :579-628).  Per sample and group of cg = C / 32 channels x HW pixels, n = cg HW elements:
    mean = sum x / n,  var = sum x^2 / n - mean^2 (biased; clamped at 0),  rstd = 1 / sqrt(var + float32(1e-6)),
    scale[c] = rstd gamma[c] out_mul,  shift[c] = (beta[c] - mean rstd gamma[c]) out_mul.
The comparator is an interval, not a tolerance.  L is the longest fp32 addition chain of the launch: a thread of k_gn_stats adds ceil(HW / lanes) pixels (:540-544,
lanes = 256 / (C / 8)), a channel thread the `lanes` partial sums (:551), a group thread cg <= C / 32 channel sums (:558), and four links stand for the scalar tail (the
rounded reciprocal 1 / n, the two products with it, the conversion of n): L = ceil(HW / lanes) + lanes + C / 32 + 4.  k_gn_finalize adds tps tile rows (:603-607) and
qpg = C / 128 quads (:619): L = max(tps0, tps1) + C / 128 + 4.  Every link errs by at most u times a partial sum of absolute values, so
    |mean_k - mean| <= dm = L u mean|x|,      |q_k - E[x^2]| <= dq = (L + 2) u E[x^2]   (the squares of bf16 values are exact in fp32; two links to spare),
    |var_k - var|   <= dv = dq + 2 |mean| dm + dm^2 + 2u (E[x^2] + mean^2)              (the product mean mean and the subtraction, fused or not, :561 / :621),
    rstd_k in [(var + dv + eps)^-1/2, (max(var - dv, 0) + eps)^-1/2] widened by 4u       (the addition of eps, sqrtf, the division: correctly rounded, one u to spare),
and scale, shift follow by interval arithmetic (products by the four corners) with one u per rounding of :569-572 / :623-626: rstd gamma, times out_mul; mean_k in
[mean - dm, mean + dm] times that product, beta minus it, times out_mul.  For k_gn_finalize the `x` are the fp32 table entries: mean|x| is sum |P.x| / n.
The epsilon is visible only where var is small: the `eps_1e-5` mutant is asserted on `randn` (a few radii) and `tiny` (10^5 radii), not on `mean8` / `const`, which
are there for the cancellation E[x^2] - mean^2 and the clamp (both kernels run all six families).  Exact tables (entries multiples of 1/4, every sum below 2^22): the
group SUMS are exact in any order; the quotients by n are exact too only where n = cg HW is a power of two -- at C = 384 (n = 144) and HW = 20, 30, 40 the
reciprocal 1 / n is rounded.  Either way the table must lie within 1e-5 of max |table| of the fp64 one, the bound tests/test_gpu_gn_partials.py states for the
producer-written tables (measured: 0.016 of it).

k_gn_fold (vae_engine.inc:62-77): sums of `fold` consecutive tile rows.  Exact family (multiples of 1/4, sums below 2^22): the fp64 sum bit for bit.  Random family:
within fold u sum |p| (fold - 1 additions in any order).

k_gn_apply (ncsnpp_kernels.h:642-744).  Per element v = x scale + shift (one fma, or a product and a sum: |v_k - v| <= dv = u (|x scale| + |v|), :684 / :730), y = act(v).
SiLU is silu_fast (:162): v rcp(1 + exp2(-v log2 e)).  For the accuracy of v_exp_f32 / v_rcp_f32 the figure used is the one AMD's public CDNA
instruction-set guides give for both, 1 ulp = 2u (the code's own comment at :161 says the same of v_rcp_f32).  The exponent -v log2(e) is rounded twice (the constant,
the product): e = exp(-v) carries (2 |v| + 2) u relatively, 1 + e one rounding, which reaches the quotient weighted by e / (1 + e) = s; the reciprocal 2u, the final
product u:  dy = 1.1 dv + |y| (s (2 |v| + 2) + 4) u   (|silu'| <= 1.1).
Down mode (:714-743): the fp64 mean of the four activated values, radius the mean of the four dy plus 3u mean|y_i| (three fp32 additions; the product with 1/4 is
exact) -- ONE rounding to bf16, so a mutant that rounds each term first fails; xr the mean of the four raw values within 3u mean|x_i|.  Up mode: every source pixel
2 x 2.  xr at mode none / up: the bytes of x.  The border of a padded output: the bit pattern 0x0000.
Pruning rule of the (C, side, mode, pad, act, xr, ld) product: every combination an engine launches -- NCSN++ res-blocks (SiLU, pad 1; none without xr at each C,
up / down with xr at C <= 256), its attention block (no act, pad 0), the `ddpm` Upsample (no act, up, pad 1), the VAE (SiLU, none / up, pad 1, no xr) -- at the side
where its paths differ (32: the ragged last row block of 34 padded rows; 8 and 4: lanes beyond the padded width), ld = C + 64 on one of each mode, and one case of each
remaining (mode, pad, act, xr) value at C = 64, side 4.

k_head_conv (head_conv.h:25-115), 32 x 32 x 128 -> 3.  Exact family: x in {0, 1, 2, 3}, scale -8, shift -40: t in {-40 .. -64}, 1 + 2^t = 1 in fp32, the activation is t,
a bf16 value; weights in {-1, -1/2, 0, 1/2, 1}, integer bias: every partial sum is a multiple of 1/2 below 2^23 and the output equals fp64 bit for bit, whatever the order.
One-hot family: one weight 1.0, bias 0: the output is the kernel's own bf16 activation of one shifted pixel (0 outside the image), held to g(t) = t / (1 + 2^t),
    dg = 1.1 u (|x scale| + |t|) + |g| (2 s + 4) u,  s = 2^t / (1 + 2^t)      (:75-78: fma, exp2 2u weighted by s, 1 + e, rcp 2u, the product).
Random family, tables and weights made by k_gn_stats (out_mul = -log2 e) and k_pack_conv (wmul = -ln 2) as the engine does: the reference is the fp64 convolution of
SiLU(GroupNorm(x)) with the unrounded weights (g w' = h w exactly: -log2 e x -ln 2 = 1), the radius
    sum over the 1,152 terms of |w'| (2^-9 |g| + dg') + |g| (2^-9 + 2u) |w'|  +  2 x 1152 u sum |g w'|  +  u |out|,
dg' = dg + 1.1 (|x| r_scale + r_shift) with the table radii of the interval above; the accumulation term is K u sum |terms| for K round-to-nearest additions in any order,
doubled because the matrix core's internal accumulation is not documented as round-to-nearest.  Two more terms stand for the float32 constants against the reference's
plain SiLU and unrounded weights: float32(-log2 e) float32(-ln 2) = 1 up to 2u (2u |h| |w| per term), and 2^(c v) with c = float32(-log2 e) is exp(-v (1 + e)), |e| <= u,
which moves the sigmoid by v s (1 - s) u (u v^2 s (1 - s) |w| per term).  A bound, wide by construction: the indexing rests on the first two families.

k_time_embed (ncsnpp_kernels.h:777-785): y = sin | cos (a), a = label exp(-h kc), kc = float32(float32(9.210340371976184) / 63), h = 0 .. 63.  The fp32 product h kc errs
by u h kc <= 9.3u in the exponent, expf by 1 ulp = 2u, the product with the label by u: |a_k - a| <= 13u |a|, which enters sin and cos at full size; sinf / cosf are
taken at 2 ulp = 4u |y|: the single-precision accuracy table of ROCm's HIP documentation ("HIP math API") bounds sinf and cosf by 2 ulp or less over the whole range and
expf by 1 ulp.  Little rests on the exact figure: the kernel's worst error is 0.27 of delta over 8,200 labels in [0, 999], and the 13u |a| term carries most of delta there.  delta = 13u |a| + 4u |y|.  The half bf16 ulp of the output is not part of delta.

Glue kernels (k_stem_im2col, k_pack_conv, k_pack_transpose, k_nhwc_to_nchw_f32): the bytes of a numpy gather with the same rounding (f32_to_bf16_bits)."""
import functools

import numpy as np

from row_kernel_cases import U, rne_bf16, bf16_bits_to_f64, f32_to_bf16_bits, half_ulp_bf16

F = np.float32
EPS = float(F(1e-6))
LOG2E_F = F(1.4426950408889634)
NEG_LOG2E = float(F(-1.4426950408889634))
NEG_LN2_F = F(-0.6931471805599453)
B = 3
SENTINEL = 0x7b7b                    # a finite bf16 pattern (3.26e36) no case produces
RS_NONE, RS_UP, RS_DOWN = 0, 1, 2
GN_ROWS = 4


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def bf(v):
    """fp64 -> the nearest bf16 value, as fp64"""
    return rne_bf16(v)


def bits_of(v):
    """bf16 VALUES (fp64 or fp32) -> their bits"""
    return f32_to_bf16_bits(np.asarray(v).astype(F))


def in_ld(bits, ld, fill=1e4):
    """[..., C] bf16 bits -> [..., ld]: the other channels hold bf16(fill), which must not matter"""
    out = np.full(bits.shape[:-1] + (ld,), f32_to_bf16_bits(F([fill]))[0], np.uint16)
    out[..., :bits.shape[-1]] = bits
    return out


# ---- interval arithmetic ------------------------------------------------------------------------------------------------------------------------------------------

def _iv_mul(a, b):
    c = np.stack(np.broadcast_arrays(a[0] * b[0], a[0] * b[1], a[1] * b[0], a[1] * b[1]))
    return c.min(axis=0), c.max(axis=0)


def _iv_widen(a, k):
    m = np.maximum(np.abs(a[0]), np.abs(a[1])) * (k * U)
    return a[0] - m, a[1] + m


def table_interval(mean, var, mabs, L, gamma, beta, out_mul, C, eps=EPS):
    """mean, var, mabs (mean |x|): fp64 [B][32]; gamma, beta fp32 [C].  Returns {"scale": (lo, hi, ref), "shift": (lo, hi, ref)}, fp64 [B][C] (module docstring)."""
    cg = C // 32
    g, bt = gamma.astype(np.float64)[None], beta.astype(np.float64)[None]
    ex2 = var + mean ** 2
    dm = L * U * mabs
    dq = (L + 2) * U * ex2
    dv = dq + 2 * np.abs(mean) * dm + dm ** 2 + 2 * U * (ex2 + mean ** 2)
    rep = lambda a: np.repeat(a, cg, axis=-1)
    r = _iv_widen((1.0 / np.sqrt(var + dv + eps), 1.0 / np.sqrt(np.maximum(var - dv, 0.0) + eps)), 4)
    sc = _iv_widen(_iv_mul((rep(r[0]), rep(r[1])), (g, g)), 1)
    scale = _iv_widen(_iv_mul(sc, (out_mul, out_mul)), 1)
    prod = _iv_widen(_iv_mul((rep(mean - dm), rep(mean + dm)), sc), 1)
    diff = _iv_widen((bt - prod[1], bt - prod[0]), 1)
    shift = _iv_widen(_iv_mul(diff, (out_mul, out_mul)), 1)
    rr = rep(1.0 / np.sqrt(var + eps))
    return {"scale": (scale[0], scale[1], rr * g * out_mul), "shift": (shift[0], shift[1], (bt - rep(mean) * rr * g) * out_mul)}


def check_table(iv, scale, shift):
    """scale, shift: fp32 [B][C] a kernel wrote.  Returns (elements outside their interval, worst |t - ref| / (distance from ref to the interval's end on that side))."""
    bad, worst = 0, 0.0
    for name, t in (("scale", scale), ("shift", shift)):
        lo, hi, ref = iv[name]
        t = np.asarray(t, F).astype(np.float64)
        bad += int((~((t >= lo) & (t <= hi))).sum())
        room = np.where(t >= ref, hi - ref, ref - lo)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(room > 0, np.abs(t - ref) / np.where(room > 0, room, 1.0), np.where(t == ref, 0.0, np.inf))
        worst = max(worst, float(np.nan_to_num(ratio, nan=np.inf).max()))
    return bad, worst


def check_table_exact(iv, scale, shift, rel=1e-5):
    """the exact-table bound: |t - ref| <= 1e-5 max |ref table|.  Returns (elements outside, worst |t - ref| / that bound)."""
    bad, worst = 0, 0.0
    for name, t in (("scale", scale), ("shift", shift)):
        ref = iv[name][2]
        lim = rel * np.abs(ref).max()
        err = np.abs(np.asarray(t, F).astype(np.float64) - ref)
        bad += int((~(err <= lim)).sum())
        worst = max(worst, float(np.nan_to_num(err, nan=np.inf).max() / lim))
    return bad, worst


def _affine(C, seed):
    r = np.random.default_rng(seed)
    gamma = (r.uniform(0.5, 1.5, C) * np.where(r.random(C) < 0.3, -1.0, 1.0)).astype(F)
    return gamma, r.standard_normal(C).astype(F)


# ---- k_gn_stats ---------------------------------------------------------------------------------------------------------------------------------------------------

STATS_SHAPES = tuple((C, HW) for C in (128, 256, 384, 512) for HW in (16, 64, 256, 1024) if HW < 1024 or C <= 256)
STATS_FAMILIES = ("randn", "tiny", "mean8", "const", "one_hot_group", "mix")
OUT_MULS = (1.0, NEG_LOG2E)
CONST_VALUE = 1.3671875
HOT_GROUP = 5


def stats_lanes(C):
    return 256 // (C // 8)


def stats_chain(C, HW):
    lanes = stats_lanes(C)
    return -(-HW // lanes) + lanes + C // 32 + 4


@functools.lru_cache(maxsize=None)
def stats_input(C, HW, family):
    """x: bf16 values as fp64 [B][HW][C]; gamma, beta fp32 [C]"""
    r = np.random.default_rng(100003 * C + 17 * HW + STATS_FAMILIES.index(family))
    cg = C // 32
    g = r.standard_normal((B, HW, C))
    if family == "tiny": g *= 0.003
    elif family == "mean8": g += 8.0
    elif family == "const": g[:] = CONST_VALUE
    elif family == "one_hot_group":
        g[:, :, HOT_GROUP * cg:(HOT_GROUP + 1) * cg] = 0.0
        g[:, HW - 1, (HOT_GROUP + 1) * cg - 1] = 3.0
    elif family == "mix":                                      # neighbouring samples and neighbouring groups differ by 100 x
        s = np.where((np.arange(B)[:, None] + np.arange(32)[None, :]) % 2 == 1, 1.0, 0.01)
        g *= np.repeat(s, cg, axis=1)[:, None, :]
    gamma, beta = _affine(C, C + HW)
    return _freeze(dict(C=C, HW=HW, family=family, x=bf(g), gamma=gamma, beta=beta, name=f"C{C}-HW{HW}-{family}"))


def group_moments(x, C):
    """fp64 (mean, biased variance, mean |x|) per sample and group: [B][32] each"""
    xg = x.reshape(x.shape[0], x.shape[1], 32, C // 32).transpose(0, 2, 1, 3).reshape(x.shape[0], 32, -1)
    mean = xg.mean(axis=2)
    return mean, ((xg - mean[..., None]) ** 2).mean(axis=2), np.abs(xg).mean(axis=2)


@functools.lru_cache(maxsize=None)
def stats_interval(C, HW, family, out_mul):
    c = stats_input(C, HW, family)
    mean, var, mabs = group_moments(c["x"], C)
    return table_interval(mean, var, mabs, stats_chain(C, HW), c["gamma"], c["beta"], out_mul, C)


STATS_MUTANTS = ("eps_1e-5", "unbiased_variance", "group_size+1", "group_size-1", "out_mul_on_scale_only", "mean_over_HW")


def _table_tail(s, q, n, gamma, beta, out_mul, C, mutant=None):
    """the shared second half of k_gn_stats / k_gn_finalize in float32: s, q fp32 [B][32] group sums -> (scale, shift) fp32 [B][C]"""
    cg = C // 32
    inv = F(1.0) / F(n)
    mean = (s * (F(1.0) / F(n // cg) if mutant == "mean_over_HW" else inv)).astype(F)
    var = ((q * inv).astype(F) - (mean * mean).astype(F)).astype(F)
    if mutant == "unbiased_variance":
        var = (var * (F(n) / F(n - 1))).astype(F)
    var = np.where(var < 0, F(0), var).astype(F)
    rstd = (F(1.0) / np.sqrt((var + F(1e-5 if mutant == "eps_1e-5" else 1e-6)).astype(F)).astype(F)).astype(F)
    rep = lambda a: np.repeat(a, cg, axis=1)
    sc = (rep(rstd) * gamma[None]).astype(F)
    om = F(out_mul)
    scale = (sc * om).astype(F)
    shift = (beta[None] - (rep(mean) * sc).astype(F)).astype(F)
    if mutant != "out_mul_on_scale_only":
        shift = (shift * om).astype(F)
    return scale, shift


def stats_restated(c, out_mul, mutant=None):
    """k_gn_stats in numpy float32 in the kernel's summation order: a pixel lane adds pixels pl, pl + lanes, ...; a channel the lanes 0, 1, ...; a group its channels"""
    C, HW = c["C"], c["HW"]
    x = c["x"].astype(F)
    lanes, cg = stats_lanes(C), C // 32
    n_it = -(-HW // lanes)
    xp = np.zeros((B, n_it * lanes, C), F)
    xp[:, :HW] = x                                                    # (a lane that has run out of pixels adds nothing: + 0 changes no sum)
    xp = xp.reshape(B, n_it, lanes, C)
    s, q = np.zeros((B, lanes, C), F), np.zeros((B, lanes, C), F)
    for i in range(n_it):
        s = (s + xp[:, i]).astype(F)
        q = (q + (xp[:, i] * xp[:, i]).astype(F)).astype(F)
    cs, cq = np.zeros((B, C), F), np.zeros((B, C), F)
    for l in range(lanes):
        cs, cq = (cs + s[:, l]).astype(F), (cq + q[:, l]).astype(F)
    if mutant in ("group_size+1", "group_size-1"):                  # groups of cg +- 1 channels, the last ones short or empty
        w = cg + (1 if mutant == "group_size+1" else -1)
        gs, gq = np.zeros((B, 32), F), np.zeros((B, 32), F)
        for g in range(32):
            for i in range(g * w, min((g + 1) * w, C)):
                gs[:, g], gq[:, g] = gs[:, g] + cs[:, i], gq[:, g] + cq[:, i]
        scale, shift = _table_tail(gs, gq, w * HW, np.ones(32 * w, F), np.zeros(32 * w, F), 1.0, 32 * w)
        idx = np.minimum(np.arange(C) // w, 31) * w                  # channel c reads the table of group c / w
        sc = (scale[:, idx] * c["gamma"][None]).astype(F)
        mean_sc = (-shift[:, idx] * c["gamma"][None]).astype(F)      # shift of the unit table is -mean rstd
        return (sc * F(out_mul)).astype(F), ((c["beta"][None] - mean_sc).astype(F) * F(out_mul)).astype(F)
    gs, gq = np.zeros((B, 32), F), np.zeros((B, 32), F)
    for i in range(cg):
        gs, gq = (gs + cs[:, i::cg][:, :32]).astype(F), (gq + cq[:, i::cg][:, :32]).astype(F)
    return _table_tail(gs, gq, cg * HW, c["gamma"], c["beta"], out_mul, C, mutant)


# ---- k_gn_finalize ------------------------------------------------------------------------------------------------------------------------------------------------

# (quads0, quads1, tps0, tps1, HW): one source (quads1 = tps1 = 0) at every C; two sources 128 + 128, 256 + 128 (C = 384: group 21 spans both), 256 + 256
FIN_CASES = ((32, 0, 1, 0, 16), (64, 0, 2, 0, 16), (96, 0, 3, 0, 12), (128, 0, 5, 0, 20), (32, 0, 8, 0, 64), (64, 0, 64, 0, 256),
             (32, 32, 1, 2, 8), (32, 32, 2, 3, 12), (64, 32, 3, 5, 30), (64, 32, 5, 8, 40), (64, 64, 8, 64, 64), (64, 64, 64, 1, 64))
FIN_FAMILIES = ("randn", "tiny", "mean8", "const", "one_hot_group", "mix", "exact")


def fin_chain(case):
    q0, q1, t0, t1, _ = case
    return max(t0, t1) + (q0 + q1) // 32 + 4


@functools.lru_cache(maxsize=None)
def fin_case(case, family):
    """P0 fp32 [B][tps0][quads0][2] (and P1): the fp64 tile sums of an x [B][HW][C], rounded to fp32 (exact family: x multiples of 1/2, nothing to round)"""
    q0, q1, t0, t1, HW = case
    C = 4 * (q0 + q1)
    cg = C // 32
    r = np.random.default_rng(7 * FIN_CASES.index(case) + FIN_FAMILIES.index(family) + 5000)
    g = r.standard_normal((B, HW, C))
    if family == "tiny": g *= 0.003
    elif family == "mean8": g += 8.0
    elif family == "const": g[:] = CONST_VALUE                   # var = 0: the clamp of :622 and the full cancellation of E[x^2] - mean^2
    elif family == "one_hot_group":
        g[:, :, HOT_GROUP * cg:(HOT_GROUP + 1) * cg] = 0.0
        g[:, HW - 1, (HOT_GROUP + 1) * cg - 1] = 3.0
    elif family == "mix": g *= np.repeat(np.where((np.arange(B)[:, None] + np.arange(32)[None, :]) % 2 == 1, 1.0, 0.01), cg, axis=1)[:, None, :]
    x = np.rint(g * 4) / 2 if family == "exact" else bf(g)

    def parts(xs, tps):
        t = xs.reshape(B, tps, HW // tps, xs.shape[2] // 4, 4)
        return np.stack([t.sum(axis=(2, 4)), (t * t).sum(axis=(2, 4))], axis=-1).astype(F)
    P0 = parts(x[:, :, :4 * q0], t0)
    P1 = parts(x[:, :, 4 * q0:], t1) if q1 else None
    gamma, beta = _affine(C, 31 * C + t0)
    mean, var, mabs, max_sum = _fin_moments(P0, P1, C, HW)
    if family == "exact":
        x64 = x.reshape(B, HW, 32, cg).transpose(0, 2, 1, 3).reshape(B, 32, -1)
        var = ((x64 - x64.mean(axis=2, keepdims=True)) ** 2).mean(axis=2)
    return _freeze(dict(case=case, family=family, C=C, HW=HW, P0=P0, P1=P1, gamma=gamma, beta=beta, mean=mean, var=var, mabs=mabs,
                        max_sum=max_sum, name="q%d+%d-tps%d.%d-HW%d-" % case + family))


def _fin_moments(P0, P1, C, HW):
    """the reference takes the fp32 table entries as they are: fp64 (mean, variance, mean |sum entries|) per group [B][32], and the largest |sum| met"""
    cg = C // 32
    cat = lambda f: np.concatenate([f(P0.astype(np.float64)).sum(axis=1)] + ([f(P1.astype(np.float64)).sum(axis=1)] if P1 is not None else []), axis=1)
    qs, qa = cat(lambda a: a), cat(np.abs)                           # [B][quads][2]
    n = cg * HW
    grp = lambda a: a.reshape(B, 32, cg // 4).sum(axis=2)
    mean, ex2, mabs = grp(qs[..., 0]) / n, grp(qs[..., 1]) / n, grp(qa[..., 0]) / n
    return mean, np.maximum(ex2 - mean ** 2, 0.0), mabs, float(qa.max())


def fin_from_x(c, tps):
    """the one-source k_gn_finalize case of a k_gn_stats input: the fp64 quad sums of x over `tps` tiles, rounded to fp32.  Returns (case, out_mul -> interval)."""
    C, HW = c["C"], c["HW"]
    t = c["x"].reshape(B, tps, HW // tps, C // 4, 4)
    P0 = np.stack([t.sum(axis=(2, 4)), (t * t).sum(axis=(2, 4))], axis=-1).astype(F)
    mean, var, mabs, max_sum = _fin_moments(P0, None, C, HW)
    fc = _freeze(dict(case=(C // 4, 0, tps, 0, HW), C=C, HW=HW, P0=P0, P1=None, gamma=c["gamma"], beta=c["beta"], mean=mean, var=var, mabs=mabs, max_sum=max_sum))
    return fc, lambda out_mul: fin_interval(fc, out_mul)


def fin_interval(c, out_mul):
    return table_interval(c["mean"], c["var"], c["mabs"], fin_chain(c["case"]), c["gamma"], c["beta"], out_mul, c["C"])


FIN_MUTANTS = ("eps_1e-5", "unbiased_variance", "out_mul_on_scale_only", "tail_tiles_dropped", "second_source_offset_by_quads0", "sample_stride_of_source0")


def fin_restated(c, out_mul, mutant=None):
    """k_gn_finalize in numpy float32: per quad the tiles in turn (four at a time, then the tail: the same order), per group its qpg quads in turn"""
    q0, q1, t0, t1, HW = c["case"]
    C = c["C"]

    def quad_sums(P, tps):
        s = np.zeros(P.shape[:1] + P.shape[2:], F)
        for t in range(tps - tps % 4 if mutant == "tail_tiles_dropped" else tps):
            s = (s + P[:, t]).astype(F)
        return s
    s0 = quad_sums(c["P0"], t0)
    if q1:
        P1 = c["P1"]
        if mutant == "sample_stride_of_source0":                     # sample b of the second source read at b tps0 quads0 floats2 instead of b tps1 quads1
            flat = P1.reshape(-1, 2)
            P1 = np.stack([np.resize(flat[min(b * t0 * q0, len(flat) - 1):], (t1 * q1, 2)).reshape(t1, q1, 2) for b in range(B)])
        s1 = quad_sums(P1, t1)
        if mutant == "second_source_offset_by_quads0":               # P1 indexed with q instead of q - quads0
            s1 = np.roll(s1, -(q0 % q1) if q0 % q1 else 1, axis=1)
        s0 = np.concatenate([s0, s1], axis=1)
    qpg = C // 128
    gs, gq = np.zeros((B, 32), F), np.zeros((B, 32), F)
    for i in range(qpg):
        gs, gq = (gs + s0[:, i::qpg, 0]).astype(F), (gq + s0[:, i::qpg, 1]).astype(F)
    if out_mul is None:                                              # fin_unclamped_var
        return gs, gq
    return _table_tail(gs, gq, (C // 32) * HW, c["gamma"], c["beta"], out_mul, C, mutant)


def fin_unclamped_var(c):
    """float32 q / n - mean^2 of the restatement BEFORE the clamp of :622, [B][32]: negative where the one-pass variance cancels below zero"""
    gs, gq = fin_restated(c, None)
    inv = F(1.0) / F((c["C"] // 32) * c["HW"])
    mean = (gs * inv).astype(F)
    return ((gq * inv).astype(F) - (mean * mean).astype(F)).astype(F)


# ---- k_gn_fold ----------------------------------------------------------------------------------------------------------------------------------------------------

FOLD_QUADS = (32, 64, 128)
FOLD_SHAPES = ((128, 2), (320, 5), (1024, 16), (4096, 64))          # (tps, fold): 64 output rows each, as VaeBase::gn_stats folds
FOLD_B = 2


@functools.lru_cache(maxsize=None)
def fold_case(quads, tps, fold, exact):
    """P fp32 [B][tps][quads][2]; sample 1 is 100 x larger (a wrong sample stride shows)"""
    r = np.random.default_rng(quads * 10007 + tps + int(exact))
    P = r.integers(-256, 257, (FOLD_B, tps, quads, 2)).astype(np.float64) / 4 if exact else r.standard_normal((FOLD_B, tps, quads, 2))
    P[1] *= 128.0 if exact else 100.0
    P = P.astype(F)
    t = P.astype(np.float64).reshape(FOLD_B, tps // fold, fold, quads, 2)
    return _freeze(dict(quads=quads, tps=tps, fold=fold, exact=exact, P=P, y=t.sum(axis=2), delta=fold * U * np.abs(t).sum(axis=2),
                        max_sum=float(np.abs(t).sum(axis=2).max()), name=f"q{quads}-tps{tps}-fold{fold}-{'exact' if exact else 'randn'}"))


FOLD_MUTANTS = ("sample_stride_of_the_output", "lanes_of_quads_96")


def fold_restated(c, mutant=None):
    """k_gn_fold in numpy float32: lane l adds tiles l, l + lanes, ...; then lane 0 adds the lanes 1, 2, ..."""
    quads, tps, fold = c["quads"], c["tps"], c["fold"]
    lanes = 256 // quads
    P = c["P"]
    if mutant == "sample_stride_of_the_output":                      # sample b read at b (tps / fold) rows instead of b tps
        flat = P.reshape(-1, quads, 2)
        P = np.stack([flat[b * (tps // fold):b * (tps // fold) + tps] for b in range(FOLD_B)])
    t = P.reshape(FOLD_B, tps // fold, fold, quads, 2)
    out = np.zeros((FOLD_B, tps // fold, quads, 2), F)
    part = []
    for l in range(lanes + (1 if mutant == "lanes_of_quads_96" else 0)):      # mutant: one lane more than `lanes` is summed (the quads = 96 hazard, restated)
        s = np.zeros_like(out)
        for i in range(l % lanes, fold, lanes):
            s = (s + t[:, :, i]).astype(F)
        part.append(s)
    out = part[0]
    for s in part[1:]:
        out = (out + s).astype(F)
    return out


def check_fold(c, out):
    """out fp32 [B][tps / fold][quads][2].  Returns (elements outside, worst |out - y| / delta)."""
    k = np.asarray(out, F).astype(np.float64)
    err = np.abs(k - c["y"])
    if c["exact"]:
        return int((~(k == c["y"])).sum()), 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.nan_to_num(np.where(c["delta"] > 0, err / np.where(c["delta"] > 0, c["delta"], 1.0), 0.0), nan=np.inf).max())
    return int((~(err <= c["delta"])).sum()), ratio


# ---- k_gn_apply ---------------------------------------------------------------------------------------------------------------------------------------------------

ACT_NONE, ACT_SILU = 0, 1
# (C, side, mode, pad, act, xr, ld) -- the pruning rule is in the module docstring
APPLY_CASES = (
    (128, 32, RS_NONE, 1, 1, 0, 128), (128, 32, RS_NONE, 1, 1, 0, 192), (256, 8, RS_NONE, 1, 1, 0, 256), (384, 8, RS_NONE, 1, 1, 0, 384), (384, 32, RS_NONE, 1, 1, 0, 448),
    (512, 4, RS_NONE, 1, 1, 0, 512), (512, 8, RS_NONE, 1, 1, 0, 576),                                       # res-blocks, the VAE, the head of the unfused plan
    (256, 8, RS_UP, 1, 1, 1, 256), (256, 4, RS_UP, 1, 1, 1, 320), (128, 32, RS_UP, 1, 1, 0, 128),            # up-sampling res-blocks (xr); the VAE's (no xr)
    (128, 32, RS_DOWN, 1, 1, 1, 128), (256, 8, RS_DOWN, 1, 1, 1, 320), (384, 4, RS_DOWN, 1, 1, 1, 384),      # down-sampling res-blocks
    (256, 8, RS_NONE, 0, 0, 0, 256), (256, 4, RS_UP, 1, 0, 0, 256),                                         # the attention block; the `ddpm` Upsample
    (64, 4, RS_NONE, 0, 1, 1, 64), (64, 4, RS_UP, 0, 1, 1, 128), (64, 4, RS_DOWN, 0, 0, 1, 64), (64, 4, RS_DOWN, 1, 0, 0, 128), (64, 4, RS_NONE, 1, 0, 1, 64))
BIG_V = 80.0


def apply_geometry(case):
    C, side, mode, pad = case[:4]
    d = 2 * side if mode == RS_UP else (side // 2 if mode == RS_DOWN else side)
    return d, d + 2 * pad, C // 8, 256 // (C // 8)                  # destination side, padded side, chunks per pixel, pixel lanes


def _silu64(v):
    with np.errstate(over="ignore"):
        return v / (1.0 + np.exp(-v))


def act_reference(x, sc, sh, act):
    """fp64 y = act(x sc + sh) and its radius (module docstring); x [B][...][C], sc / sh [B][C]"""
    e = (slice(None),) + (None,) * (x.ndim - 2)
    xs = x * sc[e]
    v = xs + sh[e]
    dv = U * (np.abs(xs) + np.abs(v))
    if act == ACT_NONE:
        return v, dv
    y = _silu64(v)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(v))                                 # e / (1 + e), e = exp(-v)
    return y, 1.1 * dv + np.abs(y) * (s * (2 * np.abs(v) + 2) + 4) * U


@functools.lru_cache(maxsize=None)
def apply_case(case):
    C, side, mode, pad, act, xr, ld = case
    d, dp, cpp, lanes = apply_geometry(case)
    r = np.random.default_rng(APPLY_CASES.index(case) + 900)
    sc = (r.uniform(0.5, 2.0, (B, C)) * np.where(r.random((B, C)) < 0.5, -1.0, 1.0)).astype(F)
    sh = (r.uniform(3.0, 6.0, (B, C)) * np.where(r.random((B, C)) < 0.5, -1.0, 1.0)).astype(F)      # act(shift) is far from 0: a border that holds it fails
    g = 2.0 * r.standard_normal((B, side, side, C))
    # +-0, bf16 sub-normals, and |v| = 80 exactly in both directions (x = (+-80 - shift) / scale would need rounding: take scale 2, shift 4 on channel 1)
    sc[:, 1], sh[:, 1] = 2.0, 4.0
    g[:, 0, 0, 0], g[:, 0, 1, 0], g[:, 1, 0, 0], g[:, 1, 1, 0] = 0.0, -0.0, 2.0 ** -130, -(2.0 ** -133)
    g[:, 0, 0, 1], g[:, 0, 1, 1], g[:, side - 1, side - 1, 1] = 38.0, -42.0, 38.0
    x = bf(g)
    xb = bits_of(x)
    assert np.array_equal(bf16_bits_to_f64(xb), x) and xb[0, 0, 1, 0] == 0x8000
    yv, dy = act_reference(x, sc.astype(np.float64), sh.astype(np.float64), act)
    if mode == RS_UP:
        yv, dy, xr_bits = yv.repeat(2, axis=1).repeat(2, axis=2), dy.repeat(2, axis=1).repeat(2, axis=2), xb.repeat(2, axis=1).repeat(2, axis=2)
        xr_y = xr_d = None
    elif mode == RS_DOWN:
        q = lambda a: a.reshape(B, d, 2, d, 2, C)
        dy = q(dy).mean(axis=(2, 4)) + 3 * U * np.abs(q(yv)).mean(axis=(2, 4))
        yv = q(yv).mean(axis=(2, 4))
        xr_bits, xr_y, xr_d = None, q(x).mean(axis=(2, 4)), 3 * U * np.abs(q(x)).mean(axis=(2, 4))
    else:
        xr_bits, xr_y, xr_d = xb, None, None
    Y, D = np.zeros((B, dp, dp, C)), np.zeros((B, dp, dp, C))
    Y[:, pad:pad + d, pad:pad + d], D[:, pad:pad + d, pad:pad + d] = yv, dy
    border = np.ones((dp, dp), bool)
    border[pad:pad + d, pad:pad + d] = False
    return _freeze(dict(case=case, x=x, xbits=in_ld(xb, ld), scale=sc, shift=sh, Y=Y, D=D, border=border, xr_bits=xr_bits, xr_y=xr_y, xr_d=xr_d,
                        name="C%d-side%d-mode%d-pad%d-act%d-xr%d-ld%d" % case))


def check_apply(c, ybits, xrbits=None):
    """ybits uint16 [B][Hp][Wp][C], xrbits [B][Hd][Wd][C] (when the case has xr).  Returns (failing elements, worst (|k - y| - half ulp) / delta)."""
    k = bf16_bits_to_f64(ybits)
    bad = ~((k >= rne_bf16(c["Y"] - c["D"])) & (k <= rne_bf16(c["Y"] + c["D"])))
    bad[:, c["border"]] |= ybits[:, c["border"]] != 0                # the border: zero BITS
    n = int(bad.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        m = c["D"] > 0
        ratio = float(np.nan_to_num(np.where(m, np.maximum(np.abs(k - c["Y"]) - half_ulp_bf16(k), 0.0) / np.where(m, c["D"], 1.0), 0.0), nan=np.inf).max())
    if c["case"][5]:
        if c["xr_bits"] is not None:
            n += int((xrbits != c["xr_bits"]).sum())
        else:
            kx = bf16_bits_to_f64(xrbits)
            n += int((~((kx >= rne_bf16(c["xr_y"] - c["xr_d"])) & (kx <= rne_bf16(c["xr_y"] + c["xr_d"])))).sum())
    return n, ratio


APPLY_MUTANTS = ("border_holds_act_shift", "up_shift_before_pad", "down_three_taps", "down_rounds_each_term", "table_chunk_from_swapped_lane", "scale_of_sample_0")


def silu_fast32(t):
    """silu_fast in float32: t rcp(1 + exp2(-t log2 e))"""
    with np.errstate(over="ignore"):
        e = np.exp2(((-t).astype(F) * LOG2E_F).astype(F)).astype(F)
    return (t * (F(1.0) / (F(1.0) + e).astype(F)).astype(F)).astype(F)


def apply_restated(c, mutant=None):
    """k_gn_apply in numpy float32 (unfused product and sum).  Returns (y bits [B][Hp][Wp][C], xr bits or None)."""
    C, side, mode, pad, act, xr, ld = c["case"]
    d, dp, cpp, lanes = apply_geometry(c["case"])
    x = c["x"].astype(F)
    sc, sh = c["scale"], c["shift"]
    if mutant == "scale_of_sample_0":
        sc = np.broadcast_to(sc[:1], sc.shape)
    # the table entry of every destination element [Hp][Wp][C]: the thread that writes pixel (row, col) of a row block is pixel lane (flat index in the block) % lanes
    tab_c = np.broadcast_to(np.arange(C), (dp, dp, C))
    if mutant == "table_chunk_from_swapped_lane":                   # tables fetched for chunk tid / lanes while the data chunk stays tid % cpp
        rows, cols = np.meshgrid(np.arange(dp), np.arange(dp), indexing="ij")
        pl = ((rows % GN_ROWS) * dp + cols) % lanes
        tid = pl[:, :, None] * cpp + np.arange(C)[None, None, :] // 8
        tab_c = np.minimum(tid // lanes, cpp - 1) * 8 + np.arange(C)[None, None, :] % 8
    # source pixel of every interior destination pixel
    idx = np.arange(d)
    if mode == RS_UP:
        src = ((idx + pad) >> 1) - pad if mutant == "up_shift_before_pad" else idx >> 1
        src = np.clip(src, 0, side - 1)
    else:
        src = idx
    bi = np.arange(B)[:, None, None, None]
    tc = tab_c[pad:pad + d, pad:pad + d][None]

    def activated(xs):                                               # xs [B][d][d][C] raw float32 -> activated float32, with the destination's tables
        t = ((xs * sc[bi, tc]).astype(F) + sh[bi, tc]).astype(F)
        return silu_fast32(t) if act == ACT_SILU else t
    xr_bits = None
    if mode == RS_DOWN:
        taps = [x[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]
        ay, ax = np.zeros((B, d, d, C), F), np.zeros((B, d, d, C), F)
        for i, t in enumerate(taps):
            if mutant == "down_three_taps" and i == 3:
                break
            a = activated(t)
            if mutant == "down_rounds_each_term":
                a = bf16_bits_to_f64(f32_to_bf16_bits(a)).astype(F)
            ay, ax = (ay + a).astype(F), (ax + t).astype(F)
        yin, xr_bits = (ay * F(0.25)).astype(F), f32_to_bf16_bits((ax * F(0.25)).astype(F))
    else:
        xs = x[:, src][:, :, src]
        yin, xr_bits = activated(xs), bits_of(xs)
    ybits = np.zeros((B, dp, dp, C), np.uint16)
    if mutant == "border_holds_act_shift":
        z = np.zeros((B, dp, dp, C), F)
        t = ((z * sc[:, None, None, :]).astype(F) + sh[:, None, None, :]).astype(F)
        ybits[:] = f32_to_bf16_bits(silu_fast32(t) if act == ACT_SILU else t)
    ybits[:, pad:pad + d, pad:pad + d] = f32_to_bf16_bits(yin)
    return ybits, (xr_bits if xr else None)


# ---- k_head_conv --------------------------------------------------------------------------------------------------------------------------------------------------

HEAD_B, HEAD_RES, HEAD_C, HEAD_K = 2, 32, 128, 1152
HEAD_LDS = (128, 192)
HEAD_PAD_ROW = 1e4                                                   # rows 3 .. 15 of the weight buffer
# (channel, tap, output channel): both 64-channel halves, all nine taps, all three output channels
ONE_HOT = ((3, 0, 0), (69, 1, 1), (63, 2, 2), (127, 3, 0), (0, 4, 1), (64, 5, 2), (31, 6, 0), (100, 7, 1), (17, 8, 2))


def head_k(c, tap):
    return ((c >> 6) * 9 + tap) * 64 + (c & 63)


def head_pack(w):
    """w [3][128][9] (values) -> bf16 bits [16][1152] in the kernel's K order, rows 3 .. 15 holding 1e4"""
    out = np.full((16, HEAD_K), f32_to_bf16_bits(F([HEAD_PAD_ROW]))[0], np.uint16)
    cc, tt = np.meshgrid(np.arange(HEAD_C), np.arange(9), indexing="ij")
    out[:3][:, head_k(cc, tt)] = f32_to_bf16_bits(np.asarray(w, F))
    return out


def conv3x3(a, w):
    """a fp64 [B][32][32][C] (zero padding), w [3][C][9] -> [B][3][32][32]: out[n, y, x] = sum a[y + ky - 1, x + kx - 1, c] w[n, c, ky 3 + kx]"""
    Bn = a.shape[0]
    ap = np.zeros((Bn, HEAD_RES + 2, HEAD_RES + 2, a.shape[3]), a.dtype)
    ap[:, 1:-1, 1:-1] = a
    out = np.zeros((Bn, 3, HEAD_RES, HEAD_RES), a.dtype)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        out += np.einsum("byxc,nc->bnyx", ap[:, ky:ky + HEAD_RES, kx:kx + HEAD_RES], w[:, :, tap])
    return out


def g64(t):
    with np.errstate(over="ignore"):
        return t / (1.0 + np.exp2(t))


def g_radius(x, sc, t):
    with np.errstate(over="ignore"):
        s = 1.0 - 1.0 / (1.0 + np.exp2(t))
    return 1.1 * U * (np.abs(x * sc) + np.abs(t)) + np.abs(g64(t)) * (2 * s + 4) * U


@functools.lru_cache(maxsize=None)
def head_exact_case():
    r = np.random.default_rng(41)
    x = r.integers(0, 4, (HEAD_B, HEAD_RES, HEAD_RES, HEAD_C)).astype(np.float64)
    w = r.integers(-2, 3, (3, HEAD_C, 9)).astype(np.float64) / 2
    bias = np.array([7.0, -3.0, 12.0], F)
    t = x * -8.0 - 40.0
    y = conv3x3(t, w) + bias.astype(np.float64)[None, :, None, None]
    max_sum = float(conv3x3(np.abs(t), np.abs(w)).max() + 12.0)
    return _freeze(dict(x=x, xbits=bits_of(x), w=w, w16=head_pack(w), bias=bias, scale=np.full((HEAD_B, HEAD_C), -8.0, F), shift=np.full((HEAD_B, HEAD_C), -40.0, F),
                        t=t, y=y, max_sum=max_sum))


@functools.lru_cache(maxsize=None)
def head_onehot_case():
    """t = x scale + shift spread over [-100, 100], exactly 0 included (channel 3: scale 1, shift 0, some x = 0)"""
    r = np.random.default_rng(42)
    sc = (r.uniform(0.5, 2.0, (HEAD_B, HEAD_C)) * np.where(r.random((HEAD_B, HEAD_C)) < 0.5, -1.0, 1.0)).astype(F)
    sh = r.uniform(-3.0, 3.0, (HEAD_B, HEAD_C)).astype(F)
    sc[:, 3], sh[:, 3] = 1.0, 0.0
    tt = r.uniform(-100.0, 100.0, (HEAD_B, HEAD_RES, HEAD_RES, HEAD_C))
    tt[:, ::5, ::3, 3] = 0.0
    tt[:, 1, 1, :], tt[:, 2, 2, :] = 100.0, -100.0
    x = bf((tt - sh.astype(np.float64)[:, None, None, :]) / sc.astype(np.float64)[:, None, None, :])
    t = x * sc.astype(np.float64)[:, None, None, :] + sh.astype(np.float64)[:, None, None, :]
    assert (t[..., 3] == 0).any() and np.abs(t).max() < 102
    return _freeze(dict(x=x, xbits=bits_of(x), scale=sc, shift=sh, t=t, g=g64(t), dg=g_radius(x, sc.astype(np.float64)[:, None, None, :], t)))


def onehot_weights(c, tap, n):
    w = np.zeros((3, HEAD_C, 9))
    w[n, c, tap] = 1.0
    return w


def check_head_onehot(c, hot, out):
    """out fp32 [B][3][32][32].  Every value a bf16 value inside [rne(g - dg), rne(g + dg)] of the one shifted pixel (0 outside the image and on the other two output
    channels).  Returns (failing elements, worst (|k - g| - half ulp) / dg)."""
    ch, tap, n = hot
    ky, kx = divmod(tap, 3)
    G, D = np.zeros((HEAD_B, 3, HEAD_RES + 2, HEAD_RES + 2)), np.zeros((HEAD_B, 3, HEAD_RES + 2, HEAD_RES + 2))
    G[:, n, 1:-1, 1:-1], D[:, n, 1:-1, 1:-1] = c["g"][..., ch], c["dg"][..., ch]
    G, D = G[:, :, ky:ky + HEAD_RES, kx:kx + HEAD_RES], D[:, :, ky:ky + HEAD_RES, kx:kx + HEAD_RES]
    o = np.ascontiguousarray(out, F)
    k = o.astype(np.float64)
    bad = ~((k >= rne_bf16(G - D)) & (k <= rne_bf16(G + D))) | ((o.view(np.uint32) & 0xffff) != 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.nan_to_num(np.where(D > 0, np.maximum(np.abs(k - G) - half_ulp_bf16(k), 0.0) / np.where(D > 0, D, 1.0), 0.0), nan=np.inf).max())
    return int(bad.sum()), ratio


@functools.lru_cache(maxsize=None)
def head_random_input():
    r = np.random.default_rng(43)
    x = bf(r.standard_normal((HEAD_B, HEAD_RES * HEAD_RES, HEAD_C)) * r.uniform(0.5, 3.0, HEAD_C) + r.standard_normal(HEAD_C))
    gamma, beta = _affine(HEAD_C, 44)
    w = (0.05 * r.standard_normal((3, HEAD_C, 9))).astype(F)
    return _freeze(dict(x=x, xbits=bits_of(x), gamma=gamma, beta=beta, w=w, bias=r.standard_normal(3).astype(F)))


@functools.lru_cache(maxsize=None)
def head_random_reference():
    """(y fp64 [B][3][32][32], radius) of conv3x3(SiLU(GroupNorm(x)), w) + bias (module docstring)"""
    c = head_random_input()
    x = c["x"]
    mean, var, mabs = group_moments(x, HEAD_C)
    iv = table_interval(mean, var, mabs, stats_chain(HEAD_C, HEAD_RES * HEAD_RES), c["gamma"], c["beta"], NEG_LOG2E, HEAD_C)
    S, H = iv["scale"][2][:, None, :], iv["shift"][2][:, None, :]
    rS = np.maximum(iv["scale"][1] - iv["scale"][2], iv["scale"][2] - iv["scale"][0])[:, None, :]
    rH = np.maximum(iv["shift"][1] - iv["shift"][2], iv["shift"][2] - iv["shift"][0])[:, None, :]
    t = x * S + H                                                    # the folded argument, t = c v with c = float32(-log2 e)
    g = g64(t)
    dg = g_radius(x, S, t) + 1.1 * (np.abs(x) * rS + rH)
    v = t / NEG_LOG2E                                                # the plain GroupNorm output
    h = _silu64(v)
    w = c["w"].astype(np.float64)
    wp = np.abs(w * float(NEG_LN2_F))
    img = lambda a: a.reshape(HEAD_B, HEAD_RES, HEAD_RES, HEAD_C)
    y = conv3x3(img(h), w) + c["bias"].astype(np.float64)[None, :, None, None]
    terms = conv3x3(img(np.abs(g)), wp)
    rad = conv3x3(img(2.0 ** -9 * np.abs(g) + dg), wp) + (2.0 ** -9 + 2 * U) * terms + 2 * HEAD_K * U * terms + U * (np.abs(y) + terms)
    # the two float32 constants: c x float32(-ln 2) = 1 up to 2u, and 2^(c v) is exp(-v (1 + e)), |e| <= u: |v| |d sigmoid / dv| |v| u
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-v))
    rad += conv3x3(img(2 * U * np.abs(h) + U * v * v * s * (1.0 - s)), np.abs(w))
    return y, rad, iv


HEAD_MUTANTS = ("dx_dy_swapped", "halves_swapped", "border_not_zeroed", "bias_per_pixel_tile", "weights_without_ln2")


def head_restated(xv, sc, sh, w16_bits, bias, mutant=None):
    """k_head_conv in numpy float32: the bf16 activation g32(x sc + sh) parked in a zero-bordered patch, then per 64-channel half, tap and 32-channel K step one
    32-term product sum (taken in fp64, rounded once) added to the fp32 accumulator -- a model of the matrix instruction's order, exact for the exact family.
    xv fp64 [B][32][32][128] bf16 values; sc, sh fp32 [B][128]; w16_bits uint16 [16][1152].  Returns fp32 [B][3][32][32]."""
    t = ((xv.astype(F) * sc[:, None, None, :]).astype(F) + sh[:, None, None, :]).astype(F)
    with np.errstate(over="ignore"):
        a = (t * (F(1.0) / (F(1.0) + np.exp2(t).astype(F)).astype(F)).astype(F)).astype(F)
    a = bf16_bits_to_f64(f32_to_bf16_bits(a))
    Bn = a.shape[0]
    ap = np.zeros((Bn, HEAD_RES + 2, HEAD_RES + 2, HEAD_C))
    if mutant == "border_not_zeroed":
        t0 = sh[:, None, None, :].astype(F)
        with np.errstate(over="ignore"):
            ap[:] = bf16_bits_to_f64(f32_to_bf16_bits((t0 * (F(1.0) / (F(1.0) + np.exp2(t0).astype(F)))).astype(F)))
    ap[:, 1:-1, 1:-1] = a
    w = bf16_bits_to_f64(w16_bits[:3])
    acc = np.zeros((Bn, 3, HEAD_RES, HEAD_RES), F)
    for h in range(2):
        hh = 1 - h if mutant == "halves_swapped" else h
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            if mutant == "dx_dy_swapped":
                ky, kx = kx, ky
            for ks in range(2):
                cs = slice(hh * 64 + ks * 32, hh * 64 + ks * 32 + 32)
                ks_ = (h * 9 + tap) * 64 + ks * 32
                acc = (acc + np.einsum("byxc,nc->bnyx", ap[:, ky:ky + HEAD_RES, kx:kx + HEAD_RES, cs], w[:, ks_:ks_ + 32]).astype(F)).astype(F)
    if mutant == "bias_per_pixel_tile":                              # bias[(tile of 16 pixels) % 3] instead of bias[channel]
        tile = (np.arange(HEAD_RES)[:, None] * 2 + np.arange(HEAD_RES)[None, :] // 16) % 3
        return (acc + bias[tile][None, None]).astype(F)
    return (acc + bias[None, :, None, None]).astype(F)


def check_head_random(y, rad, out):
    k = np.asarray(out, F).astype(np.float64)
    err = np.abs(k - y)
    return int((~(err <= rad)).sum()), float(np.nan_to_num(err / rad, nan=np.inf).max())


def pack_conv_reference(src, dst, N, Cin, taps, dst_ld, koff, tap_stride_c, chunked, wmul, drop_wmul=False):
    """k_pack_conv on a copy of dst (uint16 [rows][dst_ld]): exactly the addressed elements become bf16(float32(src) float32(wmul))"""
    out = np.array(dst)
    nn, cc, tt = np.meshgrid(np.arange(N), np.arange(Cin), np.arange(taps), indexing="ij")
    k = ((cc >> 6) * taps + tt) * 64 + (cc & 63) if chunked else tt * tap_stride_c + cc
    v = np.asarray(src, F).reshape(N, Cin, taps)
    out[nn, koff + k] = f32_to_bf16_bits(v if drop_wmul else (v * F(wmul)).astype(F))
    return out


# (N, Cin, taps, dst_ld, koff, tap_stride_c, chunked, wmul): the head's weights; the stem's; a 1x1 shortcut segment behind nine taps in a wider row; three chunks
PACK_FORMS = ((3, 128, 9, 1152, 0, 128, 1, float(NEG_LN2_F)), (128, 3, 9, 64, 0, 3, 0, 1.0), (16, 128, 1, 1280, 1152, 128, 0, 1.0), (8, 192, 9, 1728, 0, 192, 1, 1.0))
TRANSPOSE_CASE = (40, 24, 48)                                        # K, N, dst_ld
NCHW_CASE = (2, 12, 40, 48)                                          # B, HW, C, ld


@functools.lru_cache(maxsize=None)
def pack_form_case(form):
    N, Cin, taps, dst_ld, koff, ts, chunked, wmul = form
    src = np.random.default_rng(PACK_FORMS.index(form) + 60).standard_normal((N, Cin, taps)).astype(F)
    dst = np.full((N, dst_ld), SENTINEL, np.uint16)
    return _freeze(dict(src=src, y=pack_conv_reference(src, dst, *form)))


@functools.lru_cache(maxsize=None)
def transpose_case():
    K, N, ld = TRANSPOSE_CASE
    src = np.random.default_rng(70).standard_normal((K, N)).astype(F)
    y = np.full((N, ld), SENTINEL, np.uint16)
    y[:, :K] = f32_to_bf16_bits(src.T)
    return _freeze(dict(src=src, y=y))


@functools.lru_cache(maxsize=None)
def nchw_case():
    """every finite bf16 pattern class: random bits with the exponent field below 0xff, sub-normals and both zeros included"""
    Bn, HW, C, ld = NCHW_CASE
    x = np.random.default_rng(71).integers(0, 65536, (Bn, HW, ld)).astype(np.uint16)
    x = np.where((x & 0x7f80) == 0x7f80, x & 0xbfff, x).astype(np.uint16)
    x[0, 0, :4] = (0x0000, 0x8000, 0x0001, 0x807f)
    y = (x[:, :, :C].astype(np.uint32) << 16).transpose(0, 2, 1)
    return _freeze(dict(x=x, y=np.ascontiguousarray(y)))


# ---- k_stem_im2col ------------------------------------------------------------------------------------------------------------------------------------------------

STEM_B = 2


@functools.lru_cache(maxsize=None)
def stem_case():
    """x fp32 [2][3][32][32]: the three planes differ by 100 x, the two samples differ.  y: bf16 bits [2048][64], column tap 3 + c, columns 27 .. 63 zero"""
    r = np.random.default_rng(80)
    x = (r.standard_normal((STEM_B, 3, 32, 32)) * np.array([0.01, 1.0, 100.0])[None, :, None, None]).astype(F)
    return _freeze(dict(x=x, y=stem_reference(x)))


def stem_reference(x, mutant=None):
    Bn = x.shape[0]
    xp = np.zeros((Bn, 3, 34, 34), F)
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((Bn, 32, 32, 64), np.uint16)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        if mutant == "dx_dy_swapped":
            ky, kx = kx, ky
        for ch in range(3):
            k = ch * 9 + tap if mutant == "channel_major" else tap * 3 + ch
            out[..., k] = f32_to_bf16_bits(xp[:, ch, ky:ky + 32, kx:kx + 32])
    return out.reshape(Bn * 1024, 64)


# ---- k_time_embed -------------------------------------------------------------------------------------------------------------------------------------------------

LABELS = np.array([0.0, 2.0 ** -20, 1.0, 17.25, 998.999, 999.0], F)
LABELS.setflags(write=False)
BIG_BATCH = 8200                                                     # beyond 4096 blocks of 256 threads: 8192 samples
KC = float(F(F(9.210340371976184) / F(63.0)))


def embed_reference(labels=None):
    """fp64 y [len(labels)][128] and delta (labels: fp32, default LABELS)"""
    a = (LABELS if labels is None else labels).astype(np.float64)[:, None] * np.exp(-np.arange(64)[None, :] * KC)
    y = np.concatenate([np.sin(a), np.cos(a)], axis=1)
    return y, 13 * U * np.abs(np.concatenate([a, a], axis=1)) + 4 * U * np.abs(y)


EMBED_MUTANTS = ("halves_swapped", "half_dim_64", "column_index_not_wrapped")


def embed_restated(mutant=None):
    j = np.arange(128)
    h = (j if mutant == "column_index_not_wrapped" else j & 63).astype(F)
    kc = F(9.210340371976184) / F(64.0 if mutant == "half_dim_64" else 63.0)
    a = (LABELS[:, None] * np.exp((h * -kc).astype(F)).astype(F)[None, :]).astype(F)
    first = (j < 64) != (mutant == "halves_swapped")
    return f32_to_bf16_bits(np.where(first[None, :], np.sin(a), np.cos(a)).astype(F))


def check_embed(bits, labels=None):
    """bits uint16 [len(labels)][128].  Returns (failing elements, worst ratio, worst |sin^2 + cos^2 - 1| / its bound)."""
    y, d = embed_reference(labels)
    k = bf16_bits_to_f64(bits)
    bad = ~((k >= rne_bf16(y - d)) & (k <= rne_bf16(y + d)))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.nan_to_num(np.where(d > 0, np.maximum(np.abs(k - y) - half_ulp_bf16(k), 0.0) / np.where(d > 0, d, 1.0), 0.0), nan=np.inf).max())
    s, c = k[:, :64], k[:, 64:]
    es, ec = half_ulp_bf16(s) + d[:, :64], half_ulp_bf16(c) + d[:, 64:]
    lim = 2 * (np.abs(s) * es + np.abs(c) * ec) + es ** 2 + ec ** 2
    pyth = np.abs(s * s + c * c - 1.0)
    return int(bad.sum()) + int((~(pyth <= lim)).sum()), ratio, float(np.nan_to_num(pyth / lim, nan=np.inf).max())
