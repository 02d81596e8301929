"""Inputs, fp64 references, comparators, numpy-float32 restatements and mutants for the Inception engine's kernels tested alone (csrc/inception_engine.inc and
k_inc_im2col of csrc/ncsnpp_kernels.h): tests/test_inception_kernels_host.py runs them on the CPU, tests/test_gpu_inception_kernels.py on the GPU through the
natinf_debug_inc_* entry points (include/natinf_inception.h).  numpy only.

u = 2^-24, the unit roundoff of fp32.  rne16 rounds an fp64 value to the nearest bf16 (f16 = 0) or IEEE half (f16 = 1), ties to even.  A 16-bit output k of a value
y with radius delta passes when rne16(y - delta) <= k <= rne16(y + delta): every element, no mask, no share left out (a NaN fails both comparisons).

Stem (k_inc_stem).  Reference in fp64: source coordinate max(0, (dst + 0.5) in / 299 - 0.5), bilinear taps with the upper index clamped, 2 r - 1; uint8 inputs enter
as float32(byte) / float32(255), the reference's true fp32 division.  Patch element [row][k], k = (ky 3 + kx) 3 + c, is pixel (2 oy + ky, 2 ox + kx) of the resized
image; columns 27 .. row_width - 1 are zero bits; sample b starts at row b 149 149.  Radius
    delta = 2 (3u (fy + 1) Gy + 3u (fx + 1) Gx) + 8u,
fy, fx the source coordinates and Gy, Gx the largest vertical / horizontal neighbour differences of the image: the fp32 coordinate (in / 299 rounded, the product, the
subtraction: 3u (f + 1) absolute) moves the sample along a piecewise-linear function whose slope is at most G, r is doubled, and the interpolation's own roundings
(1 - l, three products and two sums per axis on values in [0, 1], 2 r - 1) stay under 8u.  The two sizes that resize nothing, (299, 299) -- and any other size on the
axis where in = 299 --, give l = 0 exactly: the 299 x 299 case must equal rne16(2 x - 1) itself.
(The list of sizes reads "(300, 64), (299, 299): identity": only the second one resizes nothing -- 300 / 299 is no identity on either axis --, so (300, 64) is run
as an ordinary case, the first H beyond the "H <= 299" remark in the kernel, with the radius above, and (299, 299) as the exact one.)

Pool (k_inc_pool).  Max: the output equals the fp64 maximum of the window's valid elements as a VALUE (inputs are 16-bit values, the maximum is one of them; +-0
compare equal).  Average: y = sum / count over the valid elements (count_include_pad = False), delta = 10u sum|x| / count: eight additions, the reciprocal, the product.

Global average (k_inc_global_avg): fp64 mean, delta = HW u mean|x| (HW - 1 additions in a chain, the division), output compared as fp32.

Pack (k_inc_pack / k_inc_pack_f16): s = gamma / sqrt(var + float32(1e-3)), W'[n][(ky kw + kx) Cp + c] = w[n][c][ky][kx] s, b' = beta - mean s, zero elsewhere.
bf16: hi in [rne(W' (1 - 3u)), rne(W' (1 + 3u))], |hi + lo - W'| <= (2^-17 + 3u) |W'|.  half: deq = the power of two that puts max|W'[n]| in [0.5, 1) (1 for a zero
row; rows whose maximum lies within 8u of a power of two are redrawn), half in [rne(W' / deq (1 -+ 3u))].  Bias within 4u (|beta| + |mean s|).

im2col (k_inc_im2col): the bytes of the numpy gather."""
import functools

import numpy as np

from row_kernel_cases import U, rne_bf16, bf16_bits_to_f64, f32_to_bf16_bits, half_ulp_bf16

F = np.float32
EPS_BN = float(np.float32(1e-3))


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---- number formats -----------------------------------------------------------------------------------------------------------------------------------------------

def rne_f16(v):
    """fp64 -> the nearest IEEE half value (ties to even), returned as fp64; sub-normals kept, beyond 65504 (+ half an ulp) +-inf"""
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def f16_bits_to_f64(bits):
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float64)


def f32_to_f16_bits(v):
    """fp32 -> half bits, round to nearest even, saturating at +-65504 (inc_cvt16)"""
    return np.clip(np.ascontiguousarray(v, np.float32), -65504.0, 65504.0).astype(np.float16).view(np.uint16)


def half_ulp_f16(v):
    a = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(a)
    return np.exp2(np.maximum(np.where(a > 0, e - 1, -14), -14).astype(np.float64) - 11)


def rne16(v, f16):
    return rne_f16(v) if f16 else rne_bf16(v)


def bits_to_f64(bits, f16):
    return f16_bits_to_f64(bits) if f16 else bf16_bits_to_f64(bits)


def f32_to_bits(v, f16):
    return f32_to_f16_bits(v) if f16 else f32_to_bf16_bits(v)


def half_ulp16(v, f16):
    return half_ulp_f16(v) if f16 else half_ulp_bf16(v)


def check_interval(k, y, delta, f16):
    """k: the kernel's 16-bit values as fp64.  Returns (mask of failing elements, worst (|k - y| - half a 16-bit ulp) / delta over the elements with delta > 0)."""
    bad = ~((k >= rne16(y - delta, f16)) & (k <= rne16(y + delta, f16)))
    with np.errstate(invalid="ignore", divide="ignore"):
        m = delta > 0
        ratio = np.where(m, np.maximum(np.abs(k - y) - half_ulp16(k, f16), 0.0) / np.where(m, delta, 1.0), 0.0)
        ratio = float(np.nanmax(ratio)) if ratio.size else 0.0
    return bad, ratio


# ---- stem -----------------------------------------------------------------------------------------------------------------------------------------------------------

STEM_SIZES = ((32, 32), (40, 24), (5, 7), (1, 1), (2, 130), (640, 16), (300, 64), (299, 299))
STEM_B = 2
STEM_WMAX = 128
OUT299, PATCH = 299, 149


def _src(n_in, mode="half_pixel"):
    """fp64 source coordinate of every destination index 0 .. 298"""
    d = np.arange(OUT299, dtype=np.float64)
    if mode == "align_corners":
        return d * (n_in - 1) / (OUT299 - 1)
    return np.maximum(0.0, (d + 0.5) * n_in / OUT299 - 0.5)


def _taps(n_in):
    f = _src(n_in)
    i0 = np.floor(f).astype(np.int64)
    return f, i0, np.minimum(i0 + 1, n_in - 1), f - i0


def resize_reference(v):
    """v fp64 [B][H][W][3] -> bilinear 299 x 299 (align_corners = False) [B][299][299][3], fp64"""
    _, y0, y1, ly = _taps(v.shape[1])
    _, x0, x1, lx = _taps(v.shape[2])
    lx_ = lx[None, None, :, None]
    top = (1 - lx_) * v[:, y0][:, :, x0] + lx_ * v[:, y0][:, :, x1]
    bot = (1 - lx_) * v[:, y1][:, :, x0] + lx_ * v[:, y1][:, :, x1]
    ly_ = ly[None, :, None, None]
    return (1 - ly_) * top + ly_ * bot


def patches(img, order="tap_major"):
    """[B][299][299][3] -> [B * 149 * 149][27]: element k = (ky 3 + kx) 3 + c of row (b 149 + oy) 149 + ox is pixel (2 oy + ky, 2 ox + kx) (mutant order: c 9 + tap)"""
    B = img.shape[0]
    out = np.empty((B, PATCH, PATCH, 9, 3), img.dtype)
    for ky in range(3):
        for kx in range(3):
            out[:, :, :, ky * 3 + kx] = img[:, ky:ky + 2 * PATCH - 1:2, kx:kx + 2 * PATCH - 1:2]
    if order == "channel_major":
        out = out.transpose(0, 1, 2, 4, 3)
    return out.reshape(B * PATCH * PATCH, 27)


@functools.lru_cache(maxsize=None)
def stem_case(H, W):
    """u8 [B][H][W][3], the fp32 [B][3][H][W] input holding the same values, and the fp64 patch rows y [B*149*149][27] with their radius"""
    r = np.random.default_rng(7919 * H + W)
    u8 = r.integers(0, 256, (STEM_B, H, W, 3), dtype=np.uint8)
    if H * W >= 4:
        u8[0].reshape(-1)[:3] = (0, 255, 128)
    f32 = (u8.astype(F) / F(255.0)).astype(F)                        # the reference's true fp32 division
    v = f32.astype(np.float64)
    y = patches(2.0 * resize_reference(v) - 1.0)
    fy, fx = _src(H), _src(W)
    gy = np.abs(np.diff(v, axis=1)).reshape(STEM_B, -1).max(axis=1) if H > 1 else np.zeros(STEM_B)
    gx = np.abs(np.diff(v, axis=2)).reshape(STEM_B, -1).max(axis=1) if W > 1 else np.zeros(STEM_B)
    d = 2.0 * (3 * U * (fy[None, :, None] + 1) * gy[:, None, None] + 3 * U * (fx[None, None, :] + 1) * gx[:, None, None]) + 8 * U
    delta = patches(np.broadcast_to(d[..., None], (STEM_B, OUT299, OUT299, 3)).copy())
    return _freeze(dict(H=H, W=W, u8=u8, f32=np.ascontiguousarray(f32.transpose(0, 3, 1, 2)), y=y, delta=delta, exact=(H, W) == (OUT299, OUT299),
                        name=f"{H}x{W}"))


STEM_MUTANTS = ("align_corners", "no_clamp_at_0", "k_channel_major", "bytes_over_256", "staged_row_off_by_one")


def stem_restated(c, f16, row_width, mutant=None):
    """k_inc_stem in numpy float32, operation by operation (unfused): bits uint16 [B*149*149][row_width]"""
    H, W = c["H"], c["W"]
    v = (c["u8"].astype(F) / F(256.0 if mutant == "bytes_over_256" else 255.0)).astype(F)

    def taps(n_in):
        d = np.arange(OUT299).astype(F)
        if mutant == "align_corners":
            f = (d * (F(n_in - 1) / F(OUT299 - 1))).astype(F)
        else:
            f = ((d + F(0.5)) * (F(n_in) / F(299.0)) - F(0.5)).astype(F)
            if mutant != "no_clamp_at_0":
                f = np.where(f < 0, F(0), f).astype(F)
        i0 = f.astype(np.int32)                                         # (int)f: toward zero
        i1 = i0 + (i0 < n_in - 1)
        return i0, i1, (f - i0.astype(F)).astype(F)

    y0, y1, ly = taps(H)
    x0, x1, lx = taps(W)
    if mutant == "staged_row_off_by_one" and W <= STEM_WMAX:           # srow[j + 1] for srow[j]
        y0, y1 = np.minimum(y0 + 1, H - 1), np.minimum(y1 + 1, H - 1)
    lx_, ly_, one = lx[None, None, :, None], ly[None, :, None, None], F(1.0)
    top = (one - lx_) * v[:, y0][:, :, x0] + lx_ * v[:, y0][:, :, x1]
    bot = (one - lx_) * v[:, y1][:, :, x0] + lx_ * v[:, y1][:, :, x1]
    r = (one - ly_) * top + ly_ * bot
    out = (F(2.0) * r - one).astype(F)
    assert out.dtype == F
    p = patches(out, "channel_major" if mutant == "k_channel_major" else "tap_major")
    bits = np.zeros((p.shape[0], row_width), np.uint16)
    bits[:, :27] = f32_to_bits(p, f16)
    return bits, p


def check_stem(c, bits, f16):
    """bits uint16 [B*149*149][row_width].  Returns (number of failing elements, worst ratio); the pad columns must be zero bits, the 299 x 299 case rne16(2 x - 1)."""
    k = bits_to_f64(bits[:, :27], f16)
    bad, ratio = check_interval(k, c["y"], c["delta"], f16)
    if c["exact"]:
        bad |= k != rne16(c["y"], f16)
    return int(bad.sum()) + int(np.count_nonzero(bits[:, 27:])), ratio


# ---- pool -----------------------------------------------------------------------------------------------------------------------------------------------------------

# (stride, pad, H, W, B, C, x_ld)
POOL_GEOMS = ((2, 0, 9, 9, 2, 72, 80), (2, 0, 8, 11, 2, 72, 80), (2, 0, 3, 3, 2, 72, 80),
              (1, 1, 8, 8, 2, 72, 80), (1, 1, 5, 7, 2, 72, 80), (1, 1, 2, 2, 2, 72, 80), (1, 1, 1, 1, 2, 72, 80), (1, 1, 1, 6, 2, 72, 80),
              (2, 1, 7, 6, 2, 72, 80),
              (1, 1, 8, 8, 2, 192, 192), (2, 0, 17, 9, 2, 192, 192))        # Ho = 8, 24 chunks, B = 2: 384 threads, a ragged second block
POOL_FAMILIES = ("normal", "post_relu", "all_negative", "constant_half", "outside_hot")
HOT = 6e4


def pool_out_hw(stride, pad, H, W):
    return (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1


def _covered(stride, pad, n):
    no = (n + 2 * pad - 3) // stride + 1
    m = np.zeros(n, bool)
    for o in range(no):
        lo = o * stride - pad
        m[max(lo, 0):min(lo + 3, n)] = True
    return m


@functools.lru_cache(maxsize=None)
def pool_case(geom, family, f16):
    """x: uint16 bits [B][H][W][x_ld] (channels >= C hold NaN), xv: the values fp64 [B][H][W][C], the fp64 max / average / radius [B][Ho][Wo][C]"""
    stride, pad, H, W, B, C, x_ld = geom
    r = np.random.default_rng(POOL_GEOMS.index(geom) * 100 + POOL_FAMILIES.index(family) * 2 + f16)
    g = r.standard_normal((B, H, W, C))
    if family == "post_relu": g = np.maximum(g, 0.0)
    elif family == "all_negative": g = -np.abs(g) - 0.01
    elif family == "constant_half": g[:] = 0.5
    cy, cx = _covered(stride, pad, H), _covered(stride, pad, W)
    if family == "outside_hot":
        g[:, ~cy] = HOT
        g[:, :, ~cx] = HOT
    xv = rne16(g, f16)
    bits = np.full((B, H, W, x_ld), 0x7e00 if f16 else 0x7fc0, np.uint16)
    bits[..., :C] = f32_to_bits(xv.astype(F), f16)
    assert np.array_equal(bits_to_f64(bits[..., :C], f16), xv)
    Ho, Wo = pool_out_hw(stride, pad, H, W)
    mx = np.full((B, Ho, Wo, C), -np.inf)
    sm, sa, cnt = np.zeros((B, Ho, Wo, C)), np.zeros((B, Ho, Wo, C)), np.zeros((Ho, Wo))
    for oy in range(Ho):
        for ox in range(Wo):
            ys = [y for y in range(oy * stride - pad, oy * stride - pad + 3) if 0 <= y < H]
            xs = [x for x in range(ox * stride - pad, ox * stride - pad + 3) if 0 <= x < W]
            w = xv[:, ys][:, :, xs].reshape(B, -1, C)
            mx[:, oy, ox], sm[:, oy, ox], sa[:, oy, ox], cnt[oy, ox] = w.max(axis=1), w.sum(axis=1), np.abs(w).sum(axis=1), len(ys) * len(xs)
    cn = cnt[None, :, :, None]
    return _freeze(dict(geom=geom, family=family, f16=f16, x=bits, xv=xv, max=mx, avg=sm / cn, delta=10 * U * sa / cn, Ho=Ho, Wo=Wo,
                        has_uncovered=bool((~cy).any() or (~cx).any()), name=f"s{stride}p{pad}-{H}x{W}-C{C}-{family}-{'f16' if f16 else 'bf16'}"))


def pool_cases():
    """(geometry, family): `outside_hot` only where a cell lies outside every window"""
    out = []
    for g in POOL_GEOMS:
        unc = (~_covered(g[0], g[1], g[2])).any() or (~_covered(g[0], g[1], g[3])).any()
        out += [(g, f) for f in POOL_FAMILIES if f != "outside_hot" or unc]
    return out


POOL_MUTANTS = ("count_include_pad", "zero_pad_wins_max", "stride2_keeps_wrong_column", "last_column_dropped")


def pool_restated(c, mode, mutant=None):
    """k_inc_pool in numpy float32 in the kernel's order: every input column reduced over its (up to) three rows first (0 + r0 + r1 + r2, a missing row adds 0 /
    -inf), then (col0 + col1) + col2, times float32(1 / (rows x columns valid)).  Returns uint16 bits [B*Ho*Wo][C]."""
    stride, pad, H, W, B, C, _ = c["geom"]
    f16, Ho, Wo = c["f16"], c["Ho"], c["Wo"]
    x = c["xv"].astype(F)
    neutral = F(0.0) if (mode == 1 or mutant == "zero_pad_wins_max") else F(-np.inf)
    out = np.empty((B, Ho, Wo, C), F)
    wlim = W - 1 if mutant == "last_column_dropped" else W
    for oy in range(Ho):
        rows = [y for y in range(oy * stride - pad, oy * stride - pad + 3)]
        nvr = sum(0 <= y < H for y in rows)

        def col(xx):
            acc = np.full((B, C), F(0.0) if mode == 1 else F(-np.inf), F)
            for y in rows:
                t = x[:, y, xx] if (0 <= y < H and 0 <= xx < wlim) else np.full((B, C), neutral, F)
                acc = (acc + t).astype(F) if mode == 1 else np.maximum(acc, t)
            return acc
        for ox in range(Wo):
            x0 = ox * stride - pad
            first = x0 - 1 if (mutant == "stride2_keeps_wrong_column" and stride == 2 and ox > 0) else x0
            a, b, n = col(first), col(x0 + 1), col(x0 + 2)
            if mode == 0:
                out[:, oy, ox] = np.maximum(np.maximum(a, b), n)
            else:
                nvc = sum(0 <= xx < W for xx in (x0, x0 + 1, x0 + 2))
                inv = F(1.0) / F(9 if mutant == "count_include_pad" else nvr * nvc)
                out[:, oy, ox] = (((a + b).astype(F) + n).astype(F) * inv).astype(F)
    return f32_to_bits(out.reshape(B * Ho * Wo, C), f16)


def check_pool(c, mode, bits):
    """bits uint16 [B*Ho*Wo][C].  Returns (number of failing elements, worst ratio (average only))."""
    k = bits_to_f64(bits, c["f16"]).reshape(c["max"].shape)
    if mode == 0:
        return int((~(k == c["max"])).sum()), 0.0
    bad, ratio = check_interval(k, c["avg"], c["delta"], c["f16"])
    if c["family"] == "constant_half":
        bad |= k != 0.5
    return int(bad.sum()), ratio


# ---- global average -------------------------------------------------------------------------------------------------------------------------------------------------

GAVG_CASES = ((3, 64, 2048), (2, 1, 8), (2, 289, 40))


@functools.lru_cache(maxsize=None)
def gavg_case(B, HW, C, f16):
    r = np.random.default_rng(B * 1000003 + HW * 101 + C + f16)
    g = r.standard_normal((B, HW, C))
    g[:, :, ::2] = np.abs(g[:, :, ::2])                              # every other channel as the network's: post-ReLU
    xv = rne16(g, f16)
    return _freeze(dict(B=B, HW=HW, C=C, f16=f16, x=f32_to_bits(xv.astype(F), f16), xv=xv, y=xv.mean(axis=1), delta=HW * U * np.abs(xv).mean(axis=1),
                        name=f"B{B}-HW{HW}-C{C}-{'f16' if f16 else 'bf16'}"))


def gavg_restated(c, mutant=None):
    x = c["xv"].astype(F)
    s = np.zeros((c["B"], c["C"]), F)
    for p in range(c["HW"]):
        s = (s + x[:, p]).astype(F)
    return (s / F(c["HW"] + (1 if mutant == "average_over_HW+1" else 0))).astype(F)


def check_gavg(c, out):
    """out fp32 [B][C].  Returns (number of failing elements, worst |out - y| / delta)."""
    k = np.asarray(out, F).astype(np.float64)
    err = np.abs(k - c["y"])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.nanmax(np.where(c["delta"] > 0, err / np.where(c["delta"] > 0, c["delta"], 1.0), 0.0)))
    return int((~(err <= c["delta"])).sum()), ratio


# ---- pack -----------------------------------------------------------------------------------------------------------------------------------------------------------

# (N, Np, C, Cp, kh, kw, Kp)
PACK_GEOMS = ((32, 32, 3, 3, 3, 3, 32), (32, 32, 3, 3, 3, 3, 64), (48, 64, 40, 64, 1, 7, 448), (48, 64, 40, 64, 7, 1, 448), (64, 64, 48, 64, 5, 5, 1600),
              (80, 96, 64, 64, 1, 1, 64))


def pack_fold(w, gamma, beta, mean, var, geom, eps=EPS_BN):
    """fp64 W' [Np][Kp], b' [Np] from fp32 operands"""
    N, Np, C, Cp, kh, kw, Kp = geom
    s = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + eps)
    t = np.zeros((Np, kh * kw, Cp))
    t[:N, :, :C] = (w.astype(np.float64) * s[:, None, None, None]).transpose(0, 2, 3, 1).reshape(N, kh * kw, C)
    W = np.zeros((Np, Kp))
    W[:, :kh * kw * Cp] = t.reshape(Np, -1)
    b = np.zeros(Np)
    b[:N] = beta.astype(np.float64) - mean.astype(np.float64) * s
    return W, b, s


def _pow2_above(m):
    """the power of two p with m / p in [0.5, 1) (1 for m = 0)"""
    _, e = np.frexp(m)
    return np.where(m > 0, np.exp2(e.astype(np.float64)), 1.0)


@functools.lru_cache(maxsize=None)
def pack_case(geom):
    N, Np, C, Cp, kh, kw, Kp = geom
    r = np.random.default_rng(PACK_GEOMS.index(geom) + 4242)
    gamma = (r.uniform(0.5, 1.5, N) * np.where(r.random(N) < 0.2, -1.0, 1.0)).astype(F)
    beta, mean = r.standard_normal(N).astype(F), r.standard_normal(N).astype(F)
    var = np.exp(r.uniform(np.log(1e-4), np.log(10.0), N)).astype(F)
    var[:2] = (1e-4, 10.0)
    w = np.empty((N, C, kh, kw), F)
    for n in range(N):
        while True:                                                 # redraw a row whose maximum lies within 8u of a power of two
            w[n] = (0.1 * r.standard_normal((C, kh, kw))).astype(F)
            m = np.abs(w[n].astype(np.float64)).max() * abs(float(gamma[n])) / np.sqrt(float(var[n]) + EPS_BN)
            fr, _ = np.frexp(m)
            if min(fr - 0.5, 1.0 - fr) > 8 * U:
                break
    W, b, s = pack_fold(w, gamma, beta, mean, var, geom)
    return _freeze(dict(geom=geom, w=w, gamma=gamma, beta=beta, mean=mean, var=var, W=W, b=b, deq=_pow2_above(np.abs(W).max(axis=1)),
                        b_delta=np.concatenate([4 * U * (np.abs(beta.astype(np.float64)) + np.abs(mean.astype(np.float64) * s)), np.zeros(Np - N)]),
                        name="N%d-Np%d-C%d-Cp%d-%dx%d-Kp%d" % geom))


PACK_MUTANTS = ("eps_1e-5", "ky_kx_swapped", "lo_zero", "bias_without_mean", "half_scale_one_power_off")


def pack_restated(c, f16, mutant=None):
    """k_inc_pack (f16 = 0: returns bf16 bits [Np][2 Kp], bias) / k_inc_pack_f16 (returns half bits [Np][Kp], bias, deq) in numpy float32"""
    N, Np, C, Cp, kh, kw, Kp = c["geom"]
    s = (c["gamma"] / np.sqrt((c["var"] + F(1e-5 if mutant == "eps_1e-5" else 1e-3)).astype(F)).astype(F)).astype(F)
    w = c["w"]
    if mutant == "ky_kx_swapped":                                   # reads w[n][c][kx][ky] (a square filter)
        assert kh == kw
        w = w.transpose(0, 1, 3, 2)
    t = np.zeros((Np, kh * kw, Cp), F)
    t[:N, :, :C] = (w * s[:, None, None, None]).astype(F).transpose(0, 2, 3, 1).reshape(N, kh * kw, C)
    v = np.zeros((Np, Kp), F)
    v[:, :kh * kw * Cp] = t.reshape(Np, -1)
    bias = np.zeros(Np, F)
    bias[:N] = c["beta"] if mutant == "bias_without_mean" else (c["beta"] - (c["mean"] * s).astype(F)).astype(F)
    if not f16:
        hi = f32_to_bf16_bits(v)
        lo = f32_to_bf16_bits((v - bf16_bits_to_f64(hi).astype(F)).astype(F))
        if mutant == "lo_zero":
            lo[:] = 0
        return np.concatenate([hi, lo], axis=1), bias
    mx = np.abs(v).max(axis=1)
    scale = _pow2_above(mx.astype(np.float64)).astype(F)
    if mutant == "half_scale_one_power_off":
        scale = np.where(mx > 0, scale * F(2.0), scale).astype(F)
    return f32_to_f16_bits((v * (F(1.0) / scale)[:, None]).astype(F)), bias, scale


def check_pack(c, f16, wp, bias, deq=None):
    """wp: uint16 bits [Np][2 Kp] (bf16) or [Np][Kp] (half); bias (and deq) fp32 [Np].  Returns (dict of failure counts per check, worst ratio)."""
    W, Kp = c["W"], c["geom"][6]
    lo_, hi_ = W * (1 - 3 * U), W * (1 + 3 * U)
    lo_, hi_ = np.minimum(lo_, hi_), np.maximum(lo_, hi_)
    fails = {}
    b = np.asarray(bias, F).astype(np.float64)
    fails["bias"] = int((~(np.abs(b - c["b"]) <= c["b_delta"])).sum())
    if not f16:
        hi, lo = bf16_bits_to_f64(wp[:, :Kp]), bf16_bits_to_f64(wp[:, Kp:])
        fails["hi"] = int((~((hi >= rne_bf16(lo_)) & (hi <= rne_bf16(hi_)))).sum())
        fails["hi+lo"] = int((~(np.abs(hi + lo - W) <= (2.0 ** -17 + 3 * U) * np.abs(W))).sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = float(np.nanmax(np.where(W != 0, np.abs(hi + lo - W) / np.where(W != 0, (2.0 ** -17 + 3 * U) * np.abs(W), 1.0), 0.0)))
        return fails, ratio
    d = np.asarray(deq, F).astype(np.float64)
    fails["deq"] = int((~(d == c["deq"])).sum())
    k = f16_bits_to_f64(wp)
    t0, t1 = lo_ / c["deq"][:, None], hi_ / c["deq"][:, None]
    fails["half"] = int((~((k >= rne_f16(t0)) & (k <= rne_f16(t1)))).sum())
    t = W / c["deq"][:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.nanmax(np.where(W != 0, np.maximum(np.abs(k - t) - half_ulp_f16(k), 0.0) / np.where(W != 0, 3 * U * np.abs(t), 1.0), 0.0)))
    return fails, ratio


# ---- im2col ---------------------------------------------------------------------------------------------------------------------------------------------------------

# (B, H, W, ld, C, kh, kw, stride, ph, pw, Kp)
IM2COL_CASES = ((1, 9, 13, 32, 32, 3, 3, 1, 1, 1, 320),        # the convolution test's ragged geometries: non-square; Kp padded beyond 288
                (2, 21, 19, 96, 96, 3, 3, 2, 1, 1, 896),       # stride 2 WITH padding; Kp = 864 padded to 896
                (2, 11, 11, 48, 48, 5, 5, 1, 2, 2, 1216),      # 5 x 5, padding 2; 1200 -> 1216
                (3, 7, 9, 40, 32, 1, 7, 1, 0, 3, 224),         # 1 x 7, ld > C
                (3, 9, 7, 40, 32, 7, 1, 1, 3, 0, 256),         # 7 x 1, ld > C, Kp padded
                (2, 17, 17, 128, 128, 3, 3, 2, 0, 0, 1152),    # the encoder's and the `ddpm` plan's 3 x 3, stride 2, no padding, on an odd size
                (2, 5, 5, 16, 8, 3, 3, 2, 0, 0, 128),          # C = 8: one thread per tap; ld = 2 C; Kp = 72 -> 128
                (4, 6, 6, 64, 64, 1, 1, 1, 0, 0, 64))          # 1 x 1


@functools.lru_cache(maxsize=None)
def im2col_case(case):
    B, H, W, ld, C, kh, kw, stride, ph, pw, Kp = case
    r = np.random.default_rng(IM2COL_CASES.index(case) + 99)
    x = r.integers(1, 65536, (B, H, W, ld), dtype=np.uint16)         # any bit pattern but zero: a copied word is never mistaken for padding
    return _freeze(dict(case=case, x=x, y=im2col_reference(x, case)))


def im2col_reference(x, case, mutant=None):
    B, H, W, ld, C, kh, kw, stride, ph, pw, Kp = case
    Ho, Wo = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    xp = np.zeros((B, H + 2 * ph, W + 2 * pw, C), x.dtype)
    xp[:, ph:ph + H, pw:pw + W] = x[..., :C]
    out = np.zeros((B, Ho, Wo, Kp), x.dtype)
    for ky in range(kh):
        for kx in range(kw):
            tap = (kx * kh + ky) if mutant == "tap_order_swapped" else ky * kw + kx
            out[..., tap * C:(tap + 1) * C] = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
    return out.reshape(B * Ho * Wo, Kp)
