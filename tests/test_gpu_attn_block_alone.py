"""The 16x16 attention block of NCSN++ ALONE (natinf_debug_attn_block: the engine's own pack kernels and launches on caller-supplied operands) against fp64, for the three
plans -- 2: k_attn_blk256_v2 (folded matrices, the default), 1: k_attn_blk256, 0: k_qkv256 + k_attn256<true> (csrc/attn_blk256.h, attn_qkv.h, attn256.h).

Reference (`_ref64`): AttnBlockpp written from its formula (layerspp.py:75-91) in fp64 on the bf16-rounded x and the fp32 weights / GroupNorm tables:
h = x sc + sh; q, k, v = h W_i + b_i; P = softmax(q k^T / 16); out = (x + (P v) W_3 + b_3) out_scale.
Rounding model (`_model64`, reference side too: it never calls the library): the same formula with a bf16 round wherever the plan's kernels round --
plans 0 / 1: h, the four packed matrices, q, k, v, the normalised P, O = P v, the output; plan 2: h, Wqk = W_0 W_1^T and Wvo = W_2 W_3 (folded in fp64, then bf16),
A' = h Wqk + cq, the normalised P, U = P h, the output (the k bias drops out of the softmax; cq = b_0 W_1^T and bo = b_2 W_3 + b_3 stay fp32 in the kernel, unrounded here).

Bound per case and plan: err = max|got - ref| / max|ref| <= 2 err_model + 2^-8 (err_model: the same figure of that plan's model, computed here on the CPU; the factor 2 covers
fp32 accumulation order and __expf, the floor is one bf16 step at the top of the output's range), and err_model <= 5e-2 is asserted first (test_rounding_models_*: no GPU),
so that the bound never becomes vacuous.

Cases (B = 3: one block per sample, three blocks exercise the sample stride; seeded generators, every input finite): see `_case`.  Figures of the CPU study
(test_rounding_models_stay_under_five_percent prints them; err_model of plan 2 / plans 1, 0): baseline 2.6e-3 / 3.1e-3, peaky 2.6e-2 / 3.5e-2, big_biases 3.0e-3 / 3.0e-3,
heavy_rows 3.2e-2 / 4.2e-2, outliers 7.5e-3 / 9.0e-3, uniform 2.4e-3 / 2.7e-3, onehot 3.6e-2 / 4.1e-2.  The factors were tuned on these figures: eight rows x 30 gives
6.0e-2 (plan 2) and x 20 gives 5.1e-2 (plan 1), so heavy_rows uses x 15.  peaky: with NIN_0 / NIN_1 scaled uniformly the logit rows are Gaussian, and the share of queries
whose fp64 top probability is >= 0.9 is a property of the row standard deviation, not of the seed -- 26 % at 6, 48 % at 10, 55 % at 12, 60 % at 14 -- so the case takes 12,
the smallest of these that covers at least half the queries (err_model stays under 3.5e-2 there); onehot takes 20 (73 % covered; 24 gives 5.4e-2 for plan 1).
The per-query arg-max check covers 55.3 % of the 768 queries in `peaky` and 72.9 % in `onehot`: each such output row must be closer (L2) to the reference row than to the row
ANY other single key would have given.

What a key-order mismatch between the score phase and the P V phase would do (test_a_key_order_mismatch_fails_the_peaky_case, CPU only: the plan's model with the columns of
P permuted in front of the P V product): un-doing the permuted key order inside every 32-key chunk (key 8 (r >> 2) + 4 h + (r & 3) taken as 16 h + r) gives err = 1.00 against
bounds of 0.056 (plan 2: x 17.7) and 0.073 (plans 1 / 0: x 13.6) and fails the arg-max check for 317 of the 425 covered queries; swapping just two keys gives the same err
(the rows of the queries that attend to them are simply wrong) and fails the arg-max check for those 4 queries.

The GPU figures of this file's run are kept in profiles/attn_block_alone/errors.txt."""
import functools
import math

import numpy as np
import pytest
import torch

B_DEFAULT = 3
PLANS = (2, 1, 0)
EPS_BF16 = 2.0 ** -8          # one bf16 step at the top of a binade, relative
OFF_FOLD_WQK, OFF_FOLD_WVO, OFF_FOLD_CQ, OFF_FOLD_BO, PACKED_BYTES, SCRATCH_PER_SAMPLE = 524288, 786432, 1048576, 1049600, 1312768, 393216      # include/natinf_ncsnpp.h


def _rb(t):
    """round to bf16 (through fp32, as the kernels' fp32 values are rounded), back in fp64"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


# --------------------------------------------------------------------------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------------------------------------------------------------------------
SIGMA_W = math.sqrt(3.0 / 256) / math.sqrt(3.0)      # std of the fan-average uniform NIN weights (256 -> 256): 0.0625, "the weight scale"
# the scale factors of the cases, tuned on the CPU so that err_model <= 5e-2 for every plan (test_rounding_models_stay_under_five_percent prints the figures)
PEAKY_STD, ONEHOT_STD, BIAS_MUL, HEAVY_MUL, TOKEN_MUL, CHANNEL_MUL = 12.0, 20.0, 10.0, 15.0, 20.0, 50.0
CASES = ("baseline", "peaky", "big_biases", "heavy_rows", "outliers", "uniform", "onehot")


def _gn_tables(x, gamma, beta):
    """GroupNorm(32 groups, eps 1e-6) of x [B][256 tokens][256 channels] in fp64 as (scale | shift) tables [B][256]: h = x * scale + shift"""
    B = x.shape[0]
    g = x.reshape(B, 256, 32, 8)
    mean = g.mean(dim=(1, 3))
    var = g.var(dim=(1, 3), unbiased=False)
    rstd = (var + 1e-6).rsqrt().repeat_interleave(8, dim=1)
    sc = gamma[None, :] * rstd
    return sc, beta[None, :] - mean.repeat_interleave(8, dim=1) * sc


@functools.lru_cache(maxsize=None)
def _case(name, B=B_DEFAULT):
    """x: fp64 holding bf16 values [B][256][256]; sc, sh: fp32 [B][256]; w: fp32 [4][256][256] ([in][out]); bias: fp32 [4][256]; out_scale.
    baseline: x ~ N(0, 1); the synthetic recipe of the block's weights (fan-average uniform + 0.01 randn, biases 0.01 randn); GroupNorm tables from x in fp64 with
      gamma = a ramp over the 64 four-channel quads (0.6 .. 1.4) x (1 + 0.1 randn), beta = 0.2 randn;
    peaky / onehot: NIN_0 and NIN_1 scaled (equally) until the fp64 logits q k^T / 16 have a per-row standard deviation of PEAKY_STD / ONEHOT_STD (onehot: out_scale 1);
    big_biases: the four biases ~ N(0, (BIAS_MUL x the weight scale)^2);   heavy_rows: eight random rows of each NIN matrix x HEAVY_MUL;
    outliers: two tokens per sample x TOKEN_MUL in sixteen channels (before the tables are computed), and one channel whose GroupNorm scale (and shift) is CHANNEL_MUL x;
    uniform: W_0 = 0, b_0 = 0: every logit equal, P = 2^-8 exactly."""
    g = torch.Generator().manual_seed({"baseline": 11, "peaky": 12, "big_biases": 13, "heavy_rows": 14, "outliers": 15, "uniform": 16, "onehot": 17}[name] + 100 * B)
    f64 = torch.float64
    x = torch.randn(B, 256, 256, generator=g, dtype=f64)
    lim = math.sqrt(3.0 / 256)
    w = (torch.rand(4, 256, 256, generator=g, dtype=f64) * 2 - 1) * lim + 0.01 * torch.randn(4, 256, 256, generator=g, dtype=f64)
    bias = 0.01 * torch.randn(4, 256, generator=g, dtype=f64)
    gamma = (0.6 + 0.8 * (torch.arange(256) // 4).to(f64) / 63) * (1 + 0.1 * torch.randn(256, generator=g, dtype=f64))
    beta = 0.2 * torch.randn(256, generator=g, dtype=f64)
    out_scale = 1.0 if name == "onehot" else 1.0 / math.sqrt(2.0)
    if name == "outliers":
        for b in range(B):
            tok = torch.randperm(256, generator=g)[:2]
            ch = torch.randperm(256, generator=g)[:16]
            x[b, tok[:, None], ch[None, :]] *= TOKEN_MUL
    x = _rb(x)
    sc, sh = _gn_tables(x, gamma, beta)
    if name == "outliers":
        c = int(torch.randint(0, 256, (1,), generator=g))
        sc[:, c] *= CHANNEL_MUL
        sh[:, c] *= CHANNEL_MUL
    if name == "big_biases":
        bias = BIAS_MUL * SIGMA_W * torch.randn(4, 256, generator=g, dtype=f64)
    if name == "heavy_rows":
        for i in range(4):
            w[i, torch.randperm(256, generator=g)[:8]] *= HEAVY_MUL
    if name == "uniform":
        w[0] = 0
        bias[0] = 0
    sc, sh = sc.to(torch.float32), sh.to(torch.float32)
    if name in ("peaky", "onehot"):
        h = x * sc.to(f64)[:, None, :] + sh.to(f64)[:, None, :]
        for _ in range(3):          # (the biases make the row std not exactly bilinear in the factor: three fixed-point steps land within a per cent)
            logits = torch.einsum("bqc,bkc->bqk", h @ w[0] + bias[0], h @ w[1] + bias[1]) / 16
            f = math.sqrt((PEAKY_STD if name == "peaky" else ONEHOT_STD) / float(logits.std(dim=-1).mean()))
            w[0] *= f
            w[1] *= f
    return {"name": name, "B": B, "x": x, "sc": sc, "sh": sh, "w": w.to(torch.float32), "bias": bias.to(torch.float32), "out_scale": out_scale}


# --------------------------------------------------------------------------------------------------------------------------------------------------------------
# fp64 reference and the plans' rounding models
# --------------------------------------------------------------------------------------------------------------------------------------------------------------
def _softmax16(s):
    return torch.softmax(s / 16, dim=-1)


def _operands(c):
    f64 = torch.float64
    return c["x"], c["sc"].to(f64)[:, None, :], c["sh"].to(f64)[:, None, :], c["w"].to(f64), c["bias"].to(f64)


@functools.lru_cache(maxsize=None)
def _ref64_cached(name, B):
    c = _case(name, B)
    x, sc, sh, w, b = _operands(c)
    h = x * sc + sh
    q, k, v = h @ w[0] + b[0], h @ w[1] + b[1], h @ w[2] + b[2]
    P = _softmax16(torch.einsum("bqc,bkc->bqk", q, k))
    out = (x + (P @ v) @ w[3] + b[3]) * c["out_scale"]
    alt = (v @ w[3] + b[3]) * c["out_scale"]          # + x[query] out_scale: the output row of a query that put all its mass on key j
    return out, P, alt


def _ref64(c):
    return _ref64_cached(c["name"], c["B"])


def _model64(c, plan, key_perm=None):
    """the plan's rounding model; key_perm (a permutation of the 256 keys): the columns of P taken in another key order than the rows of the P V operand -- what a
    disagreement between the two phases' key orders would compute"""
    x, sc, sh, w, b = _operands(c)
    h = _rb(x * sc + sh)
    if plan == 2:
        wqk, wvo = _rb(w[0] @ w[1].T), _rb(w[2] @ w[3])
        cq, bo = b[0] @ w[1].T, b[2] @ w[3] + b[3]
        a = _rb(h @ wqk + cq)
        P = _rb(_softmax16(torch.einsum("bqc,bkc->bqk", a, h)))
        if key_perm is not None:
            P = P[:, :, key_perm]
        return _rb((x + _rb(P @ h) @ wvo + bo) * c["out_scale"])
    wr = _rb(w)
    q, k, v = _rb(h @ wr[0] + b[0]), _rb(h @ wr[1] + b[1]), _rb(h @ wr[2] + b[2])
    P = _rb(_softmax16(torch.einsum("bqc,bkc->bqk", q, k)))
    if key_perm is not None:
        P = P[:, :, key_perm]
    return _rb((x + _rb(P @ v) @ wr[3] + b[3]) * c["out_scale"])


def _rel_err(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def _err_model(name, B, plan):
    c = _case(name, B)
    return _rel_err(_model64(c, 1 if plan == 0 else plan), _ref64(c)[0])          # (plans 1 and 0 round at the same points)


def _argmax_check(c, got):
    """queries whose fp64 top probability is >= 0.9: (covered, failed) -- failed: the output row is NOT closer to the reference row than to the row some other single key gives"""
    ref, P, alt = _ref64(c)
    top, arg = P.max(dim=-1)
    covered = top >= 0.9
    a = got - c["x"] * c["out_scale"]                                           # ||got_q - x_q s - alt_j||^2 for every (q, j)
    d_alt = (a * a).sum(-1)[:, :, None] - 2 * a @ alt.transpose(1, 2) + (alt * alt).sum(-1)[:, None, :]
    d_alt.scatter_(2, arg[:, :, None], float("inf"))
    d_ref = ((got - ref) ** 2).sum(-1)
    failed = covered & ~(d_ref < d_alt.min(dim=-1).values)
    return int(covered.sum()), int(failed.sum())


def _unpermute_chunks():
    """the kernels' score phase takes the keys of 32-key chunk c in the order key(h, r) = 32 c + 8 (r >> 2) + 4 h + (r & 3) (tile 2 c + h, row r); a P V phase that took
    them as 32 c + 16 h + r would pair probability column `key(h, r)` with operand row `16 h + r`"""
    perm = torch.empty(256, dtype=torch.long)
    for c in range(8):
        for h in range(2):
            for r in range(16):
                perm[32 * c + 16 * h + r] = 32 * c + 8 * (r >> 2) + 4 * h + (r & 3)
    return perm


# --------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the bound is not vacuous, and a key-order mismatch would fail it
# --------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_rounding_models_stay_under_five_percent(name):
    c = _case(name)
    ref, P, _ = _ref64(c)
    assert torch.isfinite(ref).all()
    share = float((P.max(dim=-1).values >= 0.9).double().mean())
    for plan in (2, 1):
        em = _err_model(name, c["B"], plan)
        cov, failed = _argmax_check(c, _model64(c, plan))
        print("%-10s plan %d: err_model %.3e   top-probability >= 0.9: %.1f %% of the queries, model rows failing the arg-max check: %d" % (name, plan, em, 100 * share, failed))
        assert em <= 5e-2, (name, plan, em)
        assert failed == 0
    if name in ("peaky", "onehot"):
        assert share >= 0.5, share
        logits_std = float((torch.log(P) - torch.log(P).mean(-1, keepdim=True)).std(dim=-1).mean())
        assert abs(logits_std / (PEAKY_STD if name == "peaky" else ONEHOT_STD) - 1) < 0.05
        assert len(torch.unique(P.argmax(-1)[0])) > 64          # the arg-max key differs per query
    if name == "uniform":
        assert torch.equal(P, torch.full_like(P, 2.0 ** -8))


@pytest.mark.parametrize("plan", [2, 1])
def test_a_key_order_mismatch_fails_the_peaky_case(plan):
    c = _case("peaky")
    ref = _ref64(c)[0]
    bound = 2 * _err_model("peaky", c["B"], plan) + EPS_BF16
    P = _ref64(c)[1]
    k0 = int(P[0, int(torch.nonzero(P[0].max(dim=-1).values >= 0.9)[0])].argmax())      # the arg-max key of sample 0's first covered query, and its neighbour
    swap = torch.arange(256)
    swap[k0], swap[(k0 + 1) % 256] = (k0 + 1) % 256, k0
    for what, perm, margin in (("32-key chunks un-permuted", _unpermute_chunks(), 10.0), ("two keys swapped", swap, 3.0)):
        bad = _model64(c, plan, key_perm=perm)
        err = _rel_err(bad, ref)
        cov, failed = _argmax_check(c, bad)
        print("peaky plan %d, %s: err %.3e = %.1f x the bound %.3e; arg-max check fails for %d of %d covered queries" % (plan, what, err, err / bound, bound, failed, cov))
        assert err > margin * bound
        assert failed > 0


# --------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _run(name, plan, B=B_DEFAULT, w8=1, x_ld=256, o_ld=256):
    """one natinf_debug_attn_block call; returns CPU tensors: out fp64 [B][256][o_ld] (bf16 values), gn_part fp32 [B][64][2] (the two halves of plan 0 / w8 = 0 kept:
    [B][2][64][2]) and the packed buffer (bytes).  Cached: every (case, plan, shape) runs once per session."""
    key = (name, plan, B, w8, x_ld, o_ld)
    if key in _RUNS:
        return _RUNS[key]
    from naturaldiffusion_amd._lib import lib, check, ptr, stream_ptr
    c = _case(name, B)
    dev = torch.device("cuda:0")
    poison_x, poison_o = 3.0e4, -7.0e3                      # finite pad values (bf16-exact enough to compare: they are written and read back as bf16)
    xd = torch.full((B * 256, x_ld), poison_x, dtype=torch.bfloat16)
    xd[:, :256] = c["x"].reshape(B * 256, 256).to(torch.bfloat16)
    xd = xd.to(dev)
    sc, sh, w, bias = c["sc"].to(dev).contiguous(), c["sh"].to(dev).contiguous(), c["w"].to(dev).contiguous(), c["bias"].to(dev).contiguous()
    packed = torch.zeros(PACKED_BYTES, dtype=torch.uint8, device=dev)
    scratch = torch.zeros(B * SCRATCH_PER_SAMPLE, dtype=torch.uint8, device=dev)
    out = torch.full((B * 256, o_ld), poison_o, dtype=torch.bfloat16, device=dev)
    halves = 2 if (plan == 0 and not w8) else 1
    part = torch.full((B, halves, 64, 2), float("nan"), dtype=torch.float32, device=dev)
    try:
        if not w8:
            check(lib.natinf_set_attn_waves8(0), "natinf_set_attn_waves8")
        check(lib.natinf_debug_attn_block(plan, B, ptr(xd), x_ld, ptr(sc), ptr(sh), ptr(w), ptr(bias), ptr(packed), ptr(scratch) if plan != 2 else None,
                                          ptr(out), o_ld, c["out_scale"], ptr(part), stream_ptr()), "natinf_debug_attn_block")
        torch.cuda.synchronize()
    finally:
        lib.natinf_set_attn_waves8(1)
    res = (out.cpu().to(torch.float64).reshape(B, 256, o_ld), part.cpu() if halves == 2 else part.cpu()[:, 0], packed.cpu(), xd.cpu())
    _RUNS[key] = res
    return res


def _check_gn_part(o, part, what):
    """part: (sum, sum of squares) of the kernel's UNROUNDED fp32 outputs per sample and quad; o: its bf16 outputs.  Each value differs from its bf16 by at most 2^-9
    relative, so |s - sum o| <= 2^-9 sum|v| <= 2^-8 sum|o| and |ss - sum o^2| <= (2^-8 + 2^-18) sum v^2 <= 2^-7 sum o^2; the fp32 summation error of 1,024 (512) terms is far below."""
    B = o.shape[0]
    q = o.reshape(B, o.shape[1], 64, 4).contiguous()          # (o: every token of a sample, or the half one partial row covers)
    s, sa, ss = q.sum(dim=(1, 3)), q.abs().sum(dim=(1, 3)), (q * q).sum(dim=(1, 3))
    p = part.to(torch.float64)
    assert torch.isfinite(p).all(), what
    assert ((p[..., 0] - s).abs() <= 2.0 ** -8 * sa).all(), (what, "sum", float(((p[..., 0] - s).abs() / sa).max()))
    assert ((p[..., 1] - ss).abs() <= 2.0 ** -7 * ss).all(), (what, "sum of squares", float(((p[..., 1] - ss).abs() / ss).max()))


def _check_fold(c, packed):
    """k_attn_fold_w's fp32 products against fp64: |err| <= 257 * 2^-24 * sum_i |a_i b_i| element by element (256 terms and the bias add)"""
    _, _, _, w, b = _operands(c)
    f = lambda off, n: packed[off:off + 4 * n].view(torch.float32).to(torch.float64)
    u = 257 * 2.0 ** -24
    for what, got, want, mag in (("Wqk", f(OFF_FOLD_WQK, 65536).reshape(256, 256), w[0] @ w[1].T, w[0].abs() @ w[1].abs().T),
                                 ("Wvo", f(OFF_FOLD_WVO, 65536).reshape(256, 256), w[2] @ w[3], w[2].abs() @ w[3].abs()),
                                 ("cq", f(OFF_FOLD_CQ, 256), b[0] @ w[1].T, b[0].abs() @ w[1].abs().T),
                                 ("bo", f(OFF_FOLD_BO, 256), b[2] @ w[3] + b[3], b[2].abs() @ w[3].abs() + b[3].abs())):
        assert torch.isfinite(got).all(), what
        assert ((got - want).abs() <= u * mag).all(), (c["name"], what, float(((got - want).abs() / (u * mag).clamp_min(1e-300)).max()))


def _check_case(name, B=B_DEFAULT):
    c = _case(name, B)
    ref = _ref64(c)[0]
    outs = {}
    for plan in PLANS:
        em = _err_model(name, B, plan)
        assert em <= 5e-2, (name, plan, em)                                    # on the CPU, before the GPU call
        out, part, packed, _ = _run(name, plan, B)
        err = _rel_err(out, ref)
        print("attn block alone  %-10s B %d plan %d: err %.3e  err_model %.3e  bound %.3e" % (name, B, plan, err, em, 2 * em + EPS_BF16))
        assert torch.isfinite(out).all() and torch.isfinite(part).all(), (name, plan)
        assert err <= 2 * em + EPS_BF16, (name, plan, err, em)
        _check_gn_part(out, part, (name, plan))
        if plan == 2:
            _check_fold(c, packed)
        if name in ("peaky", "onehot", "uniform"):
            cov, failed = _argmax_check(c, out)
            assert failed == 0, (name, plan, failed, cov)
        outs[plan] = (out, part)
    assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1]), name      # plans 1 and 0: the same bytes
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_attention_block_alone_against_fp64(name):
    outs = _check_case(name)
    if name == "uniform":
        # every query has the same attention term mean_k(h) Wvo + bo: (out / out_scale - x) differs between queries by the output's bf16 rounding only
        c = _case(name)
        top = float(_ref64(c)[0].abs().max()) / c["out_scale"]
        for plan in PLANS:
            t = outs[plan][0] / c["out_scale"] - c["x"]
            assert float((t - t.mean(dim=1, keepdim=True)).abs().max()) <= 2 * EPS_BF16 * top, plan


@pytest.mark.gpu
def test_attention_block_alone_single_sample():
    _check_case("baseline", B=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["baseline", "peaky"])
def test_two_four_wave_blocks_per_sample(name):
    """plan 0 under natinf_set_attn_waves8(0): k_attn256<true> as two blocks of 128 queries; its GroupNorm partial rows cover half a sample each"""
    c = _case(name)
    em = _err_model(name, c["B"], 0)
    out, part, _, _ = _run(name, 0, w8=0)
    err = _rel_err(out, _ref64(c)[0])
    print("attn block alone  %-10s B %d plan 0 (two 4-wave blocks): err %.3e  err_model %.3e  bound %.3e" % (name, c["B"], err, em, 2 * em + EPS_BF16))
    assert torch.isfinite(out).all() and err <= 2 * em + EPS_BF16, (err, em)
    for half in range(2):
        _check_gn_part(out[:, 128 * half:128 * half + 128], part[:, half], (name, "half", half))


@pytest.mark.gpu
@pytest.mark.parametrize("plan", PLANS)
def test_padded_rows_are_neither_read_nor_written(plan):
    """x_ld = 384, o_ld = 320 with a finite poison in both pads: the 256 columns are the bytes of the dense run, the pad of the output is untouched"""
    dense, dpart, _, _ = _run("baseline", plan)
    out, part, _, xd = _run("baseline", plan, x_ld=384, o_ld=320)
    assert torch.equal(out[:, :, :256], dense) and torch.equal(part, dpart)
    assert (out[:, :, 256:] == float(torch.tensor(-7.0e3).to(torch.bfloat16))).all()
    assert (xd[:, 256:].to(torch.float64) == float(torch.tensor(3.0e4).to(torch.bfloat16))).all()
