"""Inputs whose softmax attention is known EXACTLY, the expected output bytes, and a checker -- numpy only, no GPU and no library.

Two families (B sequences, H heads, T keys, head width hd; every tensor is [B][T][H][hd] bf16 as uint16 bit patterns):

  uniform   q = 0, so every score is exactly 0 and every valid key has probability 1 / T.  V is an indicator: column d of head h of sequence b is 1.0 at the
            single key j = (b H + h) hd + d when j < T, and 0 elsewhere.  The output of every query row is bf16(1 / T) in a column that owns a key and +0.0
            in a spare column.  A dropped key leaves a zero where bf16(1 / T) belongs, a key counted twice doubles it, and an admitted padded key (whose V is
            2^15) is a gross error.  `check_one_over_T` shows that the expected byte does not depend on how a kernel forms 1 / T.

  selector  keys are distinct +-1 code words, k_j = code(j); queries are q_i = A code(pi(i)) with pi a fixed-point-free permutation per (sequence, head) that
            crosses every tile boundary.  The matching key leads every other by gap = A (hd - max off-diagonal inner product) hd^-0.5 >= 40 nats, so row i
            of the output is V[pi(i)] -- as bytes: the leak of all the other keys is bounded by (T - 1) exp(-gap) max|V|, far below half a bf16 ulp of the
            smallest |V|.  A permuted, shifted or mis-strided key / query / value row selects another row of V.

`pack_mmdit` / `pack_dit` lay a case out as the two C entries take it (the contiguous layouts and the engines' interleaved ones, output canaries included),
`check_output` compares the bytes, and `reference_mmdit` is an fp64 softmax over a PACKED MMDiT case that can be told to make one of four mistakes -- how the
host test shows that the checker would notice them.
"""
import math

import numpy as np

LOG2E = 1.4426950408889634
MIN_GAP_NATS = 40.0
MAX_EXPONENT = 250.0          # A hd^0.5 log2(e): the largest base-2 exponent a score can take (fp32 exp2 stays finite at twice that distance)
NAN_BITS = 0x7FC0             # the canary: a bf16 quiet NaN
V_FLOOR = 2.0 ** -6           # smallest |V| of the selector family (keeps half an ulp of every value far above the leak bound)
BUGS = ("drop_key", "admit_pad", "swap_heads", "seq_stride")


def bf16_bits(x):
    """float array -> bf16 bit patterns (uint16), round to nearest even (finite inputs)"""
    x = np.asarray(x, dtype=np.float32)
    u = np.ascontiguousarray(x).reshape(-1).view(np.uint32).astype(np.uint64).reshape(x.shape)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_f32(bits):
    bits = np.asarray(bits, dtype=np.uint16)
    return (bits.reshape(-1).astype(np.uint32) << 16).view(np.float32).reshape(bits.shape)


def check_one_over_T(T):
    """the byte of 1 / T does not depend on the form: fp32 division, fp64 division and the reciprocal-multiply agree, and 1 / T sits at least 7.8e-4 (relative)
    from a bf16 rounding boundary, so a last-bit error of a hardware reciprocal cannot move it either.  Returns the bits."""
    one, t = np.float32(1.0), np.float32(T)
    a = bf16_bits(one / t)
    b = bf16_bits(np.float32(1.0 / float(T)))
    c = bf16_bits(one * (one / t))
    assert a == b == c, (T, a, b, c)
    x = 1.0 / T
    lo = float(bf16_f32(a))
    ulp = 2.0 ** (math.floor(math.log2(lo)) - 7)
    margin = min(abs(x - (lo - ulp / 2)), abs(x - (lo + ulp / 2))) / x
    assert margin >= 7.8e-4, (T, margin)
    return int(a)


class Case:
    def __init__(self, family, B, H, T, hd, q, k, v, expect, **info):
        self.family, self.B, self.H, self.T, self.hd = family, B, H, T, hd
        self.q, self.k, self.v, self.expect = q, k, v, expect           # uint16 [B][T][H][hd]
        self.info = info

    def __repr__(self):
        return f"Case({self.family}, B={self.B}, H={self.H}, T={self.T}, hd={self.hd}, {self.info})"


def uniform_case(B, H, T, hd, seed=0):
    assert B * H * hd >= T, "every key must own a column"
    rng = np.random.default_rng(seed)
    q = np.zeros((B, T, H, hd), np.uint16)
    k = bf16_bits(rng.standard_normal((B, T, H, hd)).astype(np.float32))
    col = np.arange(B * H * hd).reshape(B, 1, H, hd)                    # the key that owns column d of head h of sequence b
    own = col == np.arange(T).reshape(1, T, 1, 1)
    v = np.where(own, bf16_bits(np.float32(1.0)), np.uint16(0)).astype(np.uint16)
    expect = np.broadcast_to(np.where(col < T, np.uint16(check_one_over_T(T)), np.uint16(0)), (B, T, H, hd)).astype(np.uint16)
    assert v.astype(bool).sum() == T
    return Case("uniform", B, H, T, hd, q, k, v, np.ascontiguousarray(expect))


def _codes(rng, T, hd):
    """T distinct +-1 words of length hd (all 2^hd of them, shuffled, when T takes them all)"""
    assert T <= 2 ** hd, "the selector family needs T <= 2^hd"
    if hd <= 16:
        # short words: the 40-nat gap and the exponent bound together leave no room for near neighbours (hd = 16: the inner product may not exceed 12), so the
        # words come from the code of the largest minimum distance that has T of them -- 4: the extended Hamming code of length hd (even weight, and the XOR of
        # the set positions' indices is 0); 2: the even-weight words; 1: all words
        w = np.arange(2 ** hd)
        bits = (w[:, None] >> np.arange(hd)[None, :]) & 1
        even = bits.sum(axis=1) % 2 == 0
        synd = np.bitwise_xor.reduce(np.where(bits == 1, np.arange(hd)[None, :], 0), axis=1)
        for keep in (even & (synd == 0), even, np.ones(len(w), bool)):
            if keep.sum() >= T:
                break
        bits = bits[rng.permutation(np.flatnonzero(keep))[:T]]
        return (2 * bits - 1).astype(np.float32)
    # long words: random, a candidate is kept if its inner product with every word kept so far is at most hd/2 + hd/8 (3.8 sigma at hd = 40, 5 sigma at 64: few
    # are turned away), which leaves the power of two A = 16 inside both bounds at every width from 40 to 96
    cap = hd // 2 + hd // 8
    kept = np.empty((0, hd), np.float32)
    while len(kept) < T:
        cand = (2 * rng.integers(0, 2, size=(512, hd)) - 1).astype(np.float32)
        cand = cand[(cand @ kept.T).max(axis=1, initial=-hd) <= cap]
        g = cand @ cand.T
        ok = []
        for i in range(len(cand)):
            if not ok or g[i, ok].max() <= cap:
                ok.append(i)
        kept = np.concatenate([kept, cand[ok]])
    return kept[:T]


def _permutation(T, salt):
    """i -> (a i + c) mod T with gcd(a, T) = 1 and no fixed point; a near 0.38 T, so that neighbours land tiles apart"""
    i = np.arange(T)
    a0 = max(2, int(0.38 * T)) + 7 * salt
    for a in range(a0, a0 + T):
        if math.gcd(a, T) != 1 or a % T == 1:
            continue
        for c in (1 + salt, 1 + 3 * salt + T // 3, 5 + salt + T // 2):
            p = (a * i + c) % T
            if not (p == i).any():
                return p, a % T, c % T
    raise AssertionError("no fixed-point-free affine permutation found")


def selector_case(B, H, T, hd, seed=0, v=None):
    """v: optional [B][T][H][hd] float32 values that are exact in bf16 (the fp8 test's MX-exact blocks); default: random normal, |v| >= V_FLOOR"""
    rng = np.random.default_rng(seed)
    codes = np.stack([np.stack([_codes(rng, T, hd) for _ in range(H)]) for _ in range(B)])      # [B][H][T][hd]
    max_off = -hd
    for b in range(B):
        for h in range(H):
            g = codes[b, h] @ codes[b, h].T                              # integer inner products, exact in fp32
            np.fill_diagonal(g, -hd)
            max_off = max(max_off, int(g.max()))
    assert max_off < hd, "two equal code words"
    # A: the smallest power of two with the 40-nat gap (16 at widths 40 .. 96, 32 at 16).  Only where that breaks the exponent bound -- hd = 8 with all 256
    # words, neighbours one position apart: 64 gives 261 -- the smallest integer that has the gap, 57 (every integer up to 256 is exact in bf16, and so is
    # every product A * ip in fp32)
    need = MIN_GAP_NATS * math.sqrt(hd) / (hd - max_off)
    A = 2 ** math.ceil(math.log2(need))
    if A * math.sqrt(hd) * LOG2E >= MAX_EXPONENT:
        A = math.ceil(need)
    gap = A * (hd - max_off) / math.sqrt(hd)
    assert gap >= MIN_GAP_NATS, (A, max_off, gap)
    assert A * math.sqrt(hd) * LOG2E < MAX_EXPONENT and A <= 256, A
    given = v is not None
    if not given:
        v = rng.standard_normal((B, T, H, hd)).astype(np.float32)
        v = np.where(np.abs(v) < V_FLOOR, np.copysign(np.float32(V_FLOOR), v), v)
    vb = bf16_bits(v)
    vf = bf16_f32(vb)
    assert not given or np.array_equal(vf, np.asarray(v, np.float32)), "given values must be exact in bf16"
    leak = (T - 1) * math.exp(-gap) * float(np.abs(vf).max())
    half_ulp = float(np.abs(vf)[vf != 0].min()) * 2.0 ** -9
    assert leak <= half_ulp * 2.0 ** -10, (leak, half_ulp)
    q = np.empty((B, T, H, hd), np.float32)
    expect = np.empty((B, T, H, hd), np.uint16)
    perms = {}
    for b in range(B):
        for h in range(H):
            p, a, c = _permutation(T, b * H + h)
            perms[(b, h)] = p
            q[b, :, h] = A * codes[b, h][p]
            expect[b, :, h] = vb[b, p, h]
    k = np.ascontiguousarray(codes.transpose(0, 2, 1, 3))
    return Case("selector", B, H, T, hd, bf16_bits(q), bf16_bits(k), vb, expect, A=A, gap=gap, max_off=max_off, leak=leak, perms=perms)


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------------------

def pack_mmdit(case, engine_layout=False, k_pad=25.0, v_pad=2.0 ** 15):
    """natinf_attention_hd64_bf16's operands.  contiguous: separate q and k [B][Tp][D], o [B][Tp][D].  engine_layout: ONE [B][Tp][2D] buffer with k = q + D,
    o with ld_o = D + 8 and a sequence stride of (Tp + 3) rows, every output element pre-filled with the NaN canary.  Padded query rows are zero, padded key rows
    hold k_pad (may be NaN), padded V^T columns v_pad."""
    B, H, T, hd = case.B, case.H, case.T, case.hd
    assert hd == 64
    D, Tp = H * 64, (T + 127) // 128 * 128
    ld_qk = 2 * D if engine_layout else D
    qk = np.zeros((B, Tp, 2 * D), np.uint16)
    qk[:, :T, :D] = case.q.reshape(B, T, D)
    qk[:, :T, D:] = case.k.reshape(B, T, D)
    qk[:, T:, D:] = NAN_BITS if (isinstance(k_pad, float) and math.isnan(k_pad)) else bf16_bits(np.float32(k_pad))
    vT = np.full((B, D, Tp), bf16_bits(np.float32(v_pad)), np.uint16)
    vT[:, :, :T] = case.v.reshape(B, T, D).transpose(0, 2, 1)
    ld_o = D + 8 if engine_layout else D
    o_rows = Tp + 3 if engine_layout else Tp
    p = dict(B=B, H=H, T=T, Tp=Tp, D=D, ld_qk=ld_qk, qk_bs=Tp * ld_qk, vT=vT, ld_o=ld_o, o_bs=o_rows * ld_o,
             o=np.full((B, o_rows, ld_o), NAN_BITS, np.uint16))
    if engine_layout:
        p["q"], p["k_off"] = qk, D                                       # k = q + D elements
    else:
        p["q"], p["k"] = np.ascontiguousarray(qk[:, :, :D]), np.ascontiguousarray(qk[:, :, D:])
    return p


def pack_dit(case, gapped=False):
    """natinf_dit_attention_bf16's operands: the engine's [B*T][3D] buffer (q | k | v), o [B*T][D]; gapped: ld = 3D + 8 (the eight gap columns FINITE: the
    kernels' documented padding reads may land there) and ld_o = D + 4 with the NaN canary in the output gap."""
    B, H, T, hd = case.B, case.H, case.T, case.hd
    D = H * hd
    ld, ld_o = (3 * D + 8, D + 4) if gapped else (3 * D, D)
    buf = np.full((B * T, ld), bf16_bits(np.float32(3.0)), np.uint16)
    buf[:, :D] = case.q.reshape(B * T, D)
    buf[:, D:2 * D] = case.k.reshape(B * T, D)
    buf[:, 2 * D:3 * D] = case.v.reshape(B * T, D)
    return dict(B=B, H=H, T=T, hd=hd, D=D, ld=ld, ld_o=ld_o, qkv=buf, o=np.full((B * T, ld_o), NAN_BITS, np.uint16))


def check_output(case, o):
    """o: uint16 [B][rows >= T][ld_o >= D] as the kernel left it, having been pre-filled with the NaN canary ([B*T][ld_o] for the DiT entry).  Rows < T, columns
    < D must equal the expected bytes; columns >= D of EVERY row and rows beyond the padded sequence must still hold the canary.  (Rows T .. Tp-1 are unspecified.)"""
    B, H, T, hd = case.B, case.H, case.T, case.hd
    D = H * hd
    o = np.asarray(o)
    if o.ndim == 2:
        o = o.reshape(B, T, o.shape[1])
    assert o.dtype == np.uint16 and o.shape[0] == B and o.shape[1] >= T and o.shape[2] >= D, o.shape
    got, want = o[:, :T, :D].reshape(B, T, H, hd), case.expect
    bad = np.argwhere(got != want)
    if len(bad):
        b, t, h, d = (int(x) for x in bad[0])
        raise AssertionError(f"{case}: {len(bad)} of {want.size} output elements differ; first at sequence {b} row {t} head {h} channel {d}: "
                             f"got 0x{int(got[b, t, h, d]):04x} ({float(bf16_f32(got[b, t, h, d])):g}), want 0x{int(want[b, t, h, d]):04x} "
                             f"({float(bf16_f32(want[b, t, h, d])):g}); rows touched: {len(np.unique(bad[:, 1]))}, heads touched: {sorted(set(bad[:, 2].tolist()))[:8]}")
    Tp = (T + 127) // 128 * 128
    gap_cols, gap_rows = o[:, :, D:], o[:, Tp:, :]
    if gap_cols.size and (gap_cols != NAN_BITS).any():
        raise AssertionError(f"{case}: {int((gap_cols != NAN_BITS).sum())} gap-column elements were overwritten")
    if gap_rows.size and (gap_rows != NAN_BITS).any():
        raise AssertionError(f"{case}: {int((gap_rows != NAN_BITS).sum())} gap-row elements were overwritten")


def reference_mmdit(p, scale=0.125, bug=None):
    """fp64 softmax attention over a PACKED MMDiT case (what the kernel is documented to compute from those operands), written into a copy of p["o"] as bf16.
    bug: None, or one of BUGS -- drop_key: valid key 37 is skipped; admit_pad: key T is admitted; swap_heads: heads 0 and 1 of the output exchanged;
    seq_stride: q and k of sequence b are read at b * (qk_bs - ld_qk)."""
    assert bug is None or bug in BUGS
    B, H, T, Tp, D, ld_qk = p["B"], p["H"], p["T"], p["Tp"], p["D"], p["ld_qk"]
    flat = bf16_f32(p["q"]).astype(np.float64).reshape(-1)
    if "k" in p:
        kflat, k_off = bf16_f32(p["k"]).astype(np.float64).reshape(-1), 0
    else:
        kflat, k_off = flat, p["k_off"]
    vT = bf16_f32(p["vT"]).astype(np.float64)
    o = p["o"].copy()
    nkeys = T + 1 if bug == "admit_pad" else T
    keep = np.ones(nkeys, bool)
    if bug == "drop_key":
        keep[37] = False
    rows = np.arange(Tp)[:, None] * ld_qk + np.arange(64)[None, :]
    for b in range(B):
        base = b * (p["qk_bs"] - (ld_qk if bug == "seq_stride" else 0))
        for h in range(H):
            qh = flat[base + h * 64 + rows][:T]
            kh = kflat[base + k_off + h * 64 + rows][:nkeys][keep]
            s = qh @ kh.T * scale
            w = np.exp(s - s.max(axis=1, keepdims=True))
            w /= w.sum(axis=1, keepdims=True)
            out = w @ vT[b, h * 64:(h + 1) * 64, :nkeys][:, keep].T
            ho = (1 - h if h < 2 else h) if bug == "swap_heads" else h
            o[b, :T, ho * 64:(ho + 1) * 64] = np.where(np.isnan(out), NAN_BITS, bf16_bits(np.nan_to_num(out).astype(np.float32)))
    return o


def reference_dit(p):
    """fp64 softmax attention over a packed DiT case, as bf16 bits [B*T][ld_o] in a copy of p["o"]"""
    B, H, T, hd, D = p["B"], p["H"], p["T"], p["hd"], p["D"]
    x = bf16_f32(p["qkv"][:, :3 * D]).astype(np.float64).reshape(B, T, 3, H, hd)
    o = p["o"].copy()
    for b in range(B):
        for h in range(H):
            s = x[b, :, 0, h] @ x[b, :, 1, h].T * hd ** -0.5
            w = np.exp(s - s.max(axis=1, keepdims=True))
            w /= w.sum(axis=1, keepdims=True)
            o[b * T:(b + 1) * T, h * hd:(h + 1) * hd] = bf16_bits((w @ x[b, :, 2, h]).astype(np.float32))
    return o


# ---- the fp8 output epilogue --------------------------------------------------------------------------------------------------------------------------------

def e4m3_value(code):
    """e4m3 (fn) byte -> value"""
    code = np.asarray(code, np.int64)
    e, m = (code >> 3) & 15, code & 7
    mag = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    return np.where(code & 0x80, -mag, mag).astype(np.float32)


def mx_exact_values(B, T, H, seed=0):
    """V [B][T][H][64] float32 of MX-exact blocks: every 32-channel block is 2^s (s random in [-6, 6]) times e4m3 NORMAL values (no zero of either sign:
    a leak of 1e-20 under a zero could come out as either); the block maximum sits at one random position and is one of 288 .. 416 (mantissa 1.125 .. 1.625:
    strictly inside (1.0, 1.75), so the scale's binade and its `more than 1.75` step are unambiguous under a last-bit perturbation), every other value is
    below 256 in magnitude.  Returns (values, codes uint8 [B][T][H][64], scale bytes uint8 [B][T][H][2] = s + 127)."""
    rng = np.random.default_rng(seed)
    n = B * T * H * 2
    codes = (rng.integers(1, 15, size=(n, 32)) << 3 | rng.integers(0, 8, size=(n, 32))).astype(np.uint8)        # exponent field 1 .. 14: 2^-6 <= |x| < 256
    codes[np.arange(n), rng.integers(0, 32, size=n)] = 0x78 | rng.integers(1, 6, size=n)                          # 288, 320, 352, 384, 416
    codes |= (rng.integers(0, 2, size=(n, 32)) << 7).astype(np.uint8)
    s = rng.integers(-6, 7, size=n)
    vals = e4m3_value(codes) * np.exp2(s.astype(np.float32))[:, None]
    assert np.array_equal(bf16_f32(bf16_bits(vals)), vals)
    return (vals.reshape(B, T, H, 64), codes.reshape(B, T, H, 64), (s + 127).astype(np.uint8).reshape(B, T, H, 2))


def omx_index(b, h, t, blk, H, Tp):
    """byte offset of the scale of (sequence b, head h, row t, 32-channel block blk of the head) in the [B][H/2][Tp][4] planes (include/natinf_mmdit.h)"""
    return b * Tp * 2 * H + ((h >> 1) * Tp + t) * 4 + (h & 1) * 2 + blk


def mx_scale_byte(amax):
    """E8M0 byte of a block of magnitude amax (float32 array): the smallest power of two 2^e with amax 2^-e <= 448; an all-zero block gets 127"""
    amax = np.asarray(amax, np.float64)
    m, x = np.frexp(np.where(amax > 0, amax, 1.0))                      # amax = m 2^x, m in [0.5, 1): 2^(x - 9) maps it into [256, 512); one more halving above 448
    e = x - 9 + (m > 0.875)
    e = np.where(amax > 0, np.clip(e, -127, 127), 0)
    return (e + 127).astype(np.int64)
