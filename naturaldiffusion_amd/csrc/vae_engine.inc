// vae_engine.inc -- AutoencoderKL decoder and encoder engines (C ABI of include/natinf_vae.h); included after mmdit_engine.inc.
//
// The same building blocks as the NCSN++ engine: NHWC bf16 activations, 3x3 convolutions as LDS-DMA implicit GEMMs over
// zero-bordered inputs (written by the GroupNorm-apply pass, which also does the nearest 2x up-sampling), 1x1 shortcut
// convolutions fused into the second conv of a ResnetBlock as an extra K segment, residual adds in the GEMM epilogue.
// GroupNorm statistics come from the producing GEMM's epilogue (per-tile quad partials, folded by k_gn_fold when a sample
// has more than 64 tiles, then k_gn_finalize); below 16x16 the streaming kernel (one block per sample).  The mid-block
// attention (single head, C = 512) runs as batched GEMMs with the scores materialised (1 GiB per sample at r = 128).
//
// The encoder (VaeEncBuilder) is the same blocks the other way: k_vae_images writes the zero-bordered 64-channel picture conv_in reads, the stride-2
// convolutions run as k_inc_im2col + one GEMM (the `ddpm` plan's emit_downconv), conv_out leaves fp32 NCHW moments, k_vae_quant (vae_quant.hip) applies quant_conv,
// and natinf_vae_encode ends with the posterior kernel of ni_step.hip.
// Tested alone against fp64 (tests/test_gpu_glue_kernels.py; cases: tests/glue_kernel_cases.py): k_vae_latents, k_vae_images and k_vae_quant through natinf_debug_vae_latents /
// _vae_images / _vae_quant at the end of this file; k_gn_fold by tests/test_gpu_gn_kernels.py, k_softmax_rows_wide by tests/test_gpu_row_kernels.py.
#include "natinf_vae.h"
#include "transformer_plan.h"      // the mid-block attention's q | k, V^T and output-projection launches are its recipes

// the encoder's quant_conv pass k_vae_quant: vae_quant.hip
namespace ncsn_vq { void launch(const float* m, const float* W, const float* bias, float* out, int N, int hw, int64_t total, void* stream); }

namespace ncsn {

// z fp32 [B][C][r][r] -> post_quant_conv (1x1: W [C][C], bias) -> bf16 [B][r+2][r+2][64] with a zero border and zero
// channels >= C  (AutoencoderKL.decode applies post_quant_conv before the decoder)
__global__ void k_vae_latents(const float* __restrict__ z, const float* __restrict__ W, const float* __restrict__ bias,
                              bf16* __restrict__ y, int C, int r, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;         // over the padded output
    if (i >= total) return;
    const int c = (int)(i & 63), rp = r + 2;
    const int64_t pix = i >> 6;
    const int xx = (int)(pix % rp), yy = (int)((pix / rp) % rp); const int64_t b = pix / ((int64_t)rp * rp);
    float v = 0.f;
    if (c < C && xx >= 1 && xx <= r && yy >= 1 && yy <= r) {
        v = bias[c];
        for (int k = 0; k < C; ++k) v += W[c * C + k] * z[(((int64_t)b * C + k) * r + yy - 1) * r + xx - 1];
    }
    y[i] = (bf16)v;
}
// encoder input: images fp32 [B][3][R][R] -> bf16 [B][R+2][R+2][64] with a zero border and zero channels >= 3 (what the padded K = 576 conv_in reads).
// One thread per pixel of the padded output: eight 16-byte stores (its 128 bytes); consecutive threads read consecutive x of each plane.
__global__ __launch_bounds__(256) void k_vae_images(const float* __restrict__ img, bf16* __restrict__ y, int R, int64_t total)
{
    const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // over the padded output's pixels
    if (pix >= total) return;
    const int rp = R + 2;
    const int xx = (int)(pix % rp), yy = (int)((pix / rp) % rp); const int64_t b = pix / ((int64_t)rp * rp);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (xx >= 1 && xx <= R && yy >= 1 && yy <= R) {
        const int64_t plane = (int64_t)R * R;
        const float* p = img + (b * 3 * R + yy - 1) * R + xx - 1;
        const bf16 c0 = (bf16)p[0], c1 = (bf16)p[plane], c2 = (bf16)p[2 * plane];
        v.x = (uint32_t)__builtin_bit_cast(unsigned short, c0) | ((uint32_t)__builtin_bit_cast(unsigned short, c1) << 16);
        v.y = (uint32_t)__builtin_bit_cast(unsigned short, c2);
    }
    uint4* d = reinterpret_cast<uint4*>(y + pix * 64);
    d[0] = v;
#pragma unroll
    for (int k = 1; k < 8; ++k) d[k] = make_uint4(0u, 0u, 0u, 0u);
}
// the two input passes with the grid the plans give them (VaeBuilder / VaeEncBuilder and natinf_debug_vae_latents / natinf_debug_vae_images below)
inline void launch_vae_latents(const float* z, const float* W, const float* bias, bf16* y, int C, int r, int B, hipStream_t s)
{
    const int64_t tot = (int64_t)B * (r + 2) * (r + 2) * 64;
    hipLaunchKernelGGL(k_vae_latents, dim3(grid1d(tot, 256, 1 << 30)), dim3(256), 0, s, z, W, bias, y, C, r, tot);
}
inline void launch_vae_images(const float* img, bf16* y, int R, int B, hipStream_t s)
{
    const int64_t tot = (int64_t)B * (R + 2) * (R + 2);
    hipLaunchKernelGGL(k_vae_images, dim3(grid1d(tot, 256, 1 << 30)), dim3(256), 0, s, img, y, R, tot);
}
// (k_fill_f32: ncsnpp_kernels.h)
// partial GroupNorm tables P [B][tps][quads] (float2 = sum, sum of squares) -> [B][tps / fold][quads]; grid (tps / fold, B).
// Fixed summation order (lane-strided, then lanes ascending): deterministic.
__global__ __launch_bounds__(256) void k_gn_fold(const float2* __restrict__ P, int tps, int quads, int fold, float2* __restrict__ out)
{
    __shared__ float2 s_p[256];
    lds_poison();
    const int tid = threadIdx.x, q = tid % quads, lane = tid / quads, lanes = 256 / quads;
    const int64_t b = blockIdx.y;
    const float2* src = P + ((int64_t)b * tps + (int64_t)blockIdx.x * fold) * quads + q;
    float s = 0.f, qq = 0.f;
    for (int t = lane; t < fold; t += lanes) { const float2 v = src[(int64_t)t * quads]; s += v.x; qq += v.y; }
    s_p[tid] = make_float2(s, qq);
    __syncthreads();
    if (lane == 0) {
        for (int l = 1; l < lanes; ++l) { s += s_p[l * quads + q].x; qq += s_p[l * quads + q].y; }
        out[((int64_t)b * gridDim.x + blockIdx.x) * quads + q] = make_float2(s, qq);
    }
}
// row softmax for long rows: S fp32 [rows][T] -> P bf16, one wave per row, T % 64 == 0
__global__ __launch_bounds__(256) void k_softmax_rows_wide(const float* __restrict__ S, bf16* __restrict__ P, int T, int64_t rows)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* s = S + row * T;
    float mx = -INFINITY;
    for (int c = lane; c < T; c += 64) mx = fmaxf(mx, s[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int c = lane; c < T; c += 64) sum += __expf(s[c] - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.0f / sum;
    for (int c = lane; c < T; c += 64) P[row * T + c] = (bf16)(__expf(s[c] - mx) * inv);
}

}  // namespace ncsn

// The three row-softmax kernels alone (include/natinf_dit.h; tests/test_gpu_row_kernels.py): k_softmax_rows (ncsnpp_kernels.h), k_softmax_rows_1k (transformer_rows.h)
// and k_softmax_rows_wide above, the last of them to be defined.  Nothing but the engines' own launch shape: no kernel is instantiated for this entry.
extern "C" int natinf_debug_softmax_rows(int kind, const float* S, void* P, int T, int64_t rows, natinf_stream_t stream) {
    if (!S || !P || T <= 0 || rows <= 0 || kind < 0 || kind > 2) return NATINF_EINVAL;
    if (kind == 0 && (T > 256 || (T % 4 && T != 16))) return NATINF_EINVAL;      // the kernels' stated contracts
    if (kind == 1 && (T % 64 || T > 1024)) return NATINF_EINVAL;
    if (kind == 2 && T % 64) return NATINF_EINVAL;
    const dim3 grid((unsigned)((rows + 3) / 4));                                 // one wave per row, as every engine launches them
    if (kind == 0) hipLaunchKernelGGL(k_softmax_rows, grid, dim3(256), 0, (hipStream_t)stream, S, (bf16*)P, T, rows);
    else if (kind == 1) hipLaunchKernelGGL(k_softmax_rows_1k, grid, dim3(256), 0, (hipStream_t)stream, S, (bf16*)P, T, rows);
    else hipLaunchKernelGGL(k_softmax_rows_wide, grid, dim3(256), 0, (hipStream_t)stream, S, (bf16*)P, T, rows);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

struct natinf_vae : EngineCore {
    int Cl = 0, r = 0;
};
struct natinf_vae_enc : EngineCore {
    int Cl = 0, r = 0;
    int64_t mom_off = 0;                 // the moments' place in the workspace (bytes per image) when the caller passes none
};

namespace {

// what the decoder's and the encoder's plans share: GroupNorm tables, ResnetBlock, mid-block attention
struct VaeBase : PlanBuilder {
    explicit VaeBase(EngineCore& e) : PlanBuilder(e) {}

    struct GNp { int64_t gamma, beta; };
    GNp take_gn(int C) { const int64_t g = take(C), b = take(C); return GNp{pack_f32(g, C), pack_f32(b, C)}; }
    TRef new_act(int res, int C, int pad = 0) {
        TRef t; t.off = arena.alloc((int64_t)(res + 2 * pad) * (res + 2 * pad) * C * 2); t.C = C; t.ld = C; t.res = res; t.pad = pad;
        return t;
    }
    void pack_conv3(int64_t src, int64_t dst, int N, int Cin, int dst_ld) {
        E.packs.push_back([=](const PackCtx& p) {
            const int64_t n = (int64_t)N * Cin * 9;
            hipLaunchKernelGGL(k_pack_conv, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream, p.params + src,
                               reinterpret_cast<bf16*>(p.packed + dst), N, Cin, 9, dst_ld, 0, Cin, 1, 1.0f);
        });
    }
    // partial-statistics table of a GEMM output (res >= 16: a block tile of <= 256 rows lies inside one sample)
    struct Part { int64_t off = -1; int quads = 0, id = -1; bool valid() const { return off >= 0; } };
    int n_parts = 0;
    Part new_part(int res, int C) {
        Part p;
        if (res < 16) return p;
        p.quads = C / 4; p.id = n_parts++;
        p.off = arena.alloc((int64_t)(res * res / 64) * p.quads * 8);          // worst case: 64-row block tiles
        return p;
    }
    void free_part(Part& p) { if (p.valid()) arena.release(p.off); p = Part(); }
    // GroupNorm statistics of x -> (scale, shift) per (sample, channel); consumes x's partial table when it has one
    void gn_stats(const TRef& x, GNp gn, int64_t sc, int64_t sh, Part& part) {
        const int HW = x.res * x.res;
        if (part.valid()) {
            const Part p = part;
            const int C = x.C;
            const int64_t folded = arena.alloc((int64_t)64 * p.quads * 8);
            op([=](const Ctx& c) {
                int tps = HW / c.part_bm[p.id];
                const float2* src = c.at<float2>(p.off);
                if (tps > 64) {
                    const int fold = tps / 64;
                    hipLaunchKernelGGL(k_gn_fold, dim3(64, (unsigned)c.B), dim3(256), 0, c.stream, src, tps, p.quads, fold, c.at<float2>(folded));
                    src = c.at<float2>(folded); tps = 64;
                }
                hipLaunchKernelGGL(k_gn_finalize, dim3(c.B), dim3(256), 0, c.stream, src, tps, p.quads, (const float2*)nullptr, 0, 0, C, HW,
                                   c.w<float>(gn.gamma), c.w<float>(gn.beta), c.at<float>(sc), c.at<float>(sh), 1e-6f, 1.0f);
            });
            arena.release(folded);
            free_part(part);
            return;
        }
        op([=](const Ctx& c) {
            hipLaunchKernelGGL(k_gn_stats, dim3(c.B), dim3(256), 0, c.stream, c.act(x), x.ld, x.C, HW, c.w<float>(gn.gamma), c.w<float>(gn.beta),
                               c.at<float>(sc), c.at<float>(sh), 1e-6f, 1.0f);
        });
    }
    void gn_apply(const TRef& x, int64_t sc, int64_t sh, const TRef& y, int act, int mode) {
        const int logW = ilog2(x.res), rd = mode == RS_UP ? 2 * x.res : x.res, rows = rd + 2 * y.pad;
        op([=](const Ctx& c) {
            hipLaunchKernelGGL(k_gn_apply, dim3((unsigned)((rows + GN_ROWS - 1) / GN_ROWS), (unsigned)c.B), dim3(256), 0, c.stream, c.act(x), x.ld, x.C,
                               logW, 2 * logW, c.at<float>(sc), c.at<float>(sh), c.act(y), (bf16*)nullptr, act, mode, y.pad);
        });
    }
    // y = conv3x3(u) [+ shortcut1x1(xs)] [+ resid]: u zero-bordered; weights [cout][9*cin (+ cs)]
    Part conv(const TRef& u, int cin, int cout, int64_t w, int K, int64_t b, const TRef& y, const TRef* a1, int a1C, const TRef* resid) {
        const int res = u.res, logW = ilog2(res);
        const TRef a1r = a1 ? *a1 : TRef(), rr = resid ? *resid : TRef();
        const Part pt = new_part(res, cout);
        op([=](const Ctx& c) {
            GemmArgs g = gemm_defaults();
            g.a0 = c.act(u); g.a0_ld = u.ld; g.a0_C = cin; g.taps = 9; g.logW = logW; g.logHW = 2 * logW; g.a0_padded = 1;
            if (a1r.off >= 0) { g.a1 = c.act(a1r); g.a1_ld = a1r.ld; g.a1_C = a1C; }
            g.M = c.B * res * res; g.N = cout; g.b = c.w<bf16>(w); g.b_ld = K; g.bias_n = c.w<float>(b);
            if (rr.off >= 0) { g.resid = c.act(rr); g.resid_ld = rr.ld; }
            g.c = c.act(y); g.c_ld = y.ld;
            if (pt.valid()) { g.gn_part = c.at<float>(pt.off); g.gn_quads = pt.quads; }
            const int bm = launch_gemm(g, c.stream);
            if (pt.valid()) c.part_bm[pt.id] = bm;
        });
        return pt;
    }
    // xp: partial table of x (consumed); yp: that of the result
    TRef resnet(const TRef& x, Part& xp, int cin, int cout, Part& yp) {
        const int res = x.res;
        const GNp n1 = take_gn(cin);
        const int64_t p_c1w = take((int64_t)cout * cin * 9), p_c1b = take(cout);
        const GNp n2 = take_gn(cout);
        const int64_t p_c2w = take((int64_t)cout * cout * 9), p_c2b = take(cout);
        const bool sc_conv = cin != cout;
        const int64_t p_sw = sc_conv ? take((int64_t)cout * cin) : -1, p_sb = sc_conv ? take(cout) : -1;
        const int K1 = 9 * cin, K2 = 9 * cout + (sc_conv ? cin : 0);
        const int64_t w1 = wres((int64_t)cout * K1 * 2), w2 = wres((int64_t)cout * K2 * 2);
        pack_conv3(p_c1w, w1, cout, cin, K1);
        pack_conv3(p_c2w, w2, cout, cout, K2);
        const int64_t b1 = pack_f32(p_c1b, cout);
        int64_t b2;
        if (sc_conv) {
            E.packs.push_back([=](const PackCtx& p) {             // 1x1 shortcut weights behind the 3x3 ones, biases summed
                const int64_t n = (int64_t)cout * cin;
                hipLaunchKernelGGL(k_pack_conv, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream, p.params + p_sw,
                                   reinterpret_cast<bf16*>(p.packed + w2), cout, cin, 1, K2, 9 * cout, cin, 0, 1.0f);
            });
            b2 = wres((int64_t)cout * 4);
            E.packs.push_back([=](const PackCtx& p) {
                hipLaunchKernelGGL(k_copy_add_f32, dim3(grid1d(cout)), dim3(256), 0, p.stream, p.params + p_c2b, p.params + p_sb,
                                   reinterpret_cast<float*>(p.packed + b2), cout);
            });
        } else {
            b2 = pack_f32(p_c2b, cout);
        }
        const int64_t sc = arena.alloc((int64_t)512 * 4), sh = arena.alloc((int64_t)512 * 4);
        gn_stats(x, n1, sc, sh, xp);
        TRef u = new_act(res, cin, 1);
        gn_apply(x, sc, sh, u, ACT_SILU, RS_NONE);
        TRef t = new_act(res, cout);
        Part tp = conv(u, cin, cout, w1, K1, b1, t, nullptr, 0, nullptr);
        arena.release(u.off);
        gn_stats(t, n2, sc, sh, tp);
        TRef u2 = new_act(res, cout, 1);
        gn_apply(t, sc, sh, u2, ACT_SILU, RS_NONE);
        arena.release(t.off);
        TRef y = new_act(res, cout);
        if (sc_conv) yp = conv(u2, cout, cout, w2, K2, b2, y, &x, cin, nullptr);
        else yp = conv(u2, cout, cout, w2, K2, b2, y, nullptr, 0, &x);
        arena.release(u2.off); arena.release(sc); arena.release(sh);
        return y;
    }
    TRef attention(const TRef& x, Part& xp, Part& yp) {
        const int C = 512, res = x.res, T = res * res;
        const Part pt = new_part(res, C);
        yp = pt;
        const GNp gn = take_gn(C);
        const int64_t p_qw = take((int64_t)C * C), p_qb = take(C), p_kw = take((int64_t)C * C), p_kb = take(C);
        const int64_t p_vw = take((int64_t)C * C), p_vb = take(C), p_ow = take((int64_t)C * C), p_ob = take(C);
        const int64_t wqk = wres((int64_t)2 * C * C * 2), bqk = wres((int64_t)2 * C * 4);
        pack_bf16_at(p_qw, C, C, wqk); pack_bf16_at(p_kw, C, C, wqk + (int64_t)C * C * 2);
        pack_f32_at(p_qb, C, bqk); pack_f32_at(p_kb, C, bqk + (int64_t)C * 4);
        const int64_t wv = pack_bf16(p_vw, C, C), bv = pack_f32(p_vb, C), wo = pack_bf16(p_ow, C, C), bo = pack_f32(p_ob, C);
        const int64_t sc = arena.alloc((int64_t)C * 4), sh = arena.alloc((int64_t)C * 4);
        gn_stats(x, gn, sc, sh, xp);
        TRef h = new_act(res, C);
        gn_apply(x, sc, sh, h, ACT_NONE, RS_NONE);
        const int64_t qk = arena.alloc((int64_t)T * 2 * C * 2), vT = arena.alloc((int64_t)C * T * 2);
        const int64_t S = arena.alloc((int64_t)T * T * 4), P = arena.alloc((int64_t)T * T * 2);
        TRef O = new_act(res, C), y = new_act(res, C);
        op([=](const Ctx& c) {
            launch_gemm(dense(c, c.act(h), C, c.B * T, Lin{wqk, bqk}, 2 * C, ACT_NONE, c.at<bf16>(qk), OUT_BF16), c.stream);      // q | k
            launch_gemm(vt(c, Lin{wv, bv}, C, c.act(h), T, c.at<bf16>(vT), T), c.stream);                                       // V^T[b] = Wv h[b]^T + bv
            GemmArgs g = gemm_defaults();                       // S[b] = q k^T / sqrt(C)
            g.a0 = c.at<bf16>(qk); g.a0_ld = 2 * C; g.a0_C = C; g.a_bs = (int64_t)T * 2 * C; g.M = T; g.N = T;
            g.b = c.at<bf16>(qk) + C; g.b_ld = 2 * C; g.b_bs = (int64_t)T * 2 * C; g.scale = 1.0f / sqrtf((float)C);
            g.c = c.at<float>(S); g.c_ld = T; g.c_bs = (int64_t)T * T; g.c_mode = OUT_F32; g.batch = c.B;
            launch_gemm(g, c.stream);
            const int64_t rows = (int64_t)c.B * T;
            hipLaunchKernelGGL(k_softmax_rows_wide, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, c.stream, c.at<float>(S), c.at<bf16>(P), T, rows);
            g = gemm_defaults();                                // O[b] = P V
            g.a0 = c.at<bf16>(P); g.a0_ld = T; g.a0_C = T; g.a_bs = (int64_t)T * T; g.M = T; g.N = C;
            g.b = c.at<bf16>(vT); g.b_ld = T; g.b_bs = (int64_t)C * T; g.c = c.act(O); g.c_ld = C; g.c_bs = (int64_t)T * C; g.batch = c.B;
            launch_gemm(g, c.stream);
            g = dense(c, c.act(O), C, c.B * T, Lin{wo, bo}, C, ACT_NONE, c.act(y), OUT_BF16);      // y = x + O Wo^T + bo
            g.resid = c.act(x); g.resid_ld = x.ld;
            if (pt.valid()) { g.gn_part = c.at<float>(pt.off); g.gn_quads = pt.quads; }
            const int bm = launch_gemm(g, c.stream);
            if (pt.valid()) c.part_bm[pt.id] = bm;
        });
        arena.release(h.off); arena.release(qk); arena.release(vT); arena.release(S); arena.release(P); arena.release(O.off);
        arena.release(sc); arena.release(sh);
        return y;
    }
};

struct VaeBuilder : VaeBase {
    natinf_vae& V;
    explicit VaeBuilder(natinf_vae& e) : VaeBase(e), V(e) {}
    int64_t ident_sc = -1, ident_sh = -1;                 // scale 1 / shift 0 per (sample, channel): the plain up-sampling pass

    void build() {
        const int Cl = V.Cl, r = V.r;
        // post_quant_conv (1x1 on the latents), then conv_in: latents -> zero-bordered 64-channel NHWC, 3x3 conv to 512
        const int64_t p_qw = take((int64_t)Cl * Cl), p_qb = take(Cl);
        const int64_t wq = pack_f32(p_qw, (int64_t)Cl * Cl), bq = pack_f32(p_qb, Cl);
        const int64_t p_iw = take((int64_t)512 * Cl * 9), p_ib = take(512);
        const int64_t wi = wres((int64_t)512 * 576 * 2);
        E.packs.push_back([=](const PackCtx& p) {
            const int64_t n = (int64_t)512 * 576;
            hipLaunchKernelGGL(k_fill_bf16_zero, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream, reinterpret_cast<bf16*>(p.packed + wi), n);
        });
        pack_conv3(p_iw, wi, 512, Cl, 576);
        const int64_t bi = pack_f32(p_ib, 512);
        TRef z = new_act(r, 64, 1);
        ident_sc = arena.alloc((int64_t)512 * 4); ident_sh = arena.alloc((int64_t)512 * 4);
        const int64_t isc = ident_sc, ish = ident_sh;
        op([=](const Ctx& c) {
            launch_vae_latents(c.x, c.w<float>(wq), c.w<float>(bq), c.act(z), Cl, r, c.B, c.stream);
            const int64_t n = (int64_t)c.B * 512;
            hipLaunchKernelGGL(k_fill_f32, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, c.stream, c.at<float>(isc), 1.0f, n);
            hipLaunchKernelGGL(k_fill_f32, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, c.stream, c.at<float>(ish), 0.0f, n);
        });
        TRef x = new_act(r, 512);
        Part xp = conv(z, 64, 512, wi, 576, bi, x, nullptr, 0, nullptr), np;
        arena.release(z.off);
        auto step = [&](TRef nx) { arena.release(x.off); x = nx; free_part(xp); xp = np; np = Part(); };
        step(resnet(x, xp, 512, 512, np));
        step(attention(x, xp, np));
        step(resnet(x, xp, 512, 512, np));
        const int chans[4] = {512, 512, 256, 128};
        int cin = 512;
        for (int i = 0; i < 4; ++i) {
            const int cout = chans[i];
            for (int j = 0; j < 3; ++j) step(resnet(x, xp, j == 0 ? cin : cout, cout, np));
            if (i < 3) {                                           // nearest 2x (identity "norm" pass writes the bordered, up-sampled tensor) + conv
                const int64_t p_uw = take((int64_t)cout * cout * 9), p_ub = take(cout);
                const int64_t wu = wres((int64_t)cout * cout * 9 * 2);
                pack_conv3(p_uw, wu, cout, cout, 9 * cout);
                const int64_t bu = pack_f32(p_ub, cout);
                TRef u = new_act(2 * x.res, cout, 1);
                // scale/shift tables are [B][C] with the tensor's own C as the row length
                gn_apply_ident(x, u);
                TRef y = new_act(2 * x.res, cout);
                np = conv(u, cout, cout, wu, 9 * cout, bu, y, nullptr, 0, nullptr);
                arena.release(u.off);
                step(y);
            }
            cin = cout;
        }
        const GNp gno = take_gn(128);
        const int64_t p_ow = take((int64_t)3 * 128 * 9), p_ob = take(3);
        const int64_t wo = wres((int64_t)3 * 1152 * 2);
        pack_conv3(p_ow, wo, 3, 128, 1152);
        const int64_t bo = pack_f32(p_ob, 3);
        const int64_t sc = arena.alloc((int64_t)512 * 4), sh = arena.alloc((int64_t)512 * 4);
        gn_stats(x, gno, sc, sh, xp);
        TRef u = new_act(x.res, 128, 1);
        gn_apply(x, sc, sh, u, ACT_SILU, RS_NONE);
        const int res = x.res, logW = ilog2(res);
        op([=](const Ctx& c) {
            GemmArgs g = gemm_defaults();
            g.a0 = c.act(u); g.a0_ld = u.ld; g.a0_C = 128; g.taps = 9; g.logW = logW; g.logHW = 2 * logW; g.a0_padded = 1;
            g.M = c.B * res * res; g.N = 3; g.b = c.w<bf16>(wo); g.b_ld = 1152; g.bias_n = c.w<float>(bo);
            g.c = c.out; g.c_mode = OUT_F32_NCHW;
            launch_gemm(g, c.stream);
        });
        E.part_bm.assign(n_parts > 0 ? n_parts : 1, 128);
        finish();
    }
    // nearest 2x up-sampling of x into the zero-bordered u: the GroupNorm-apply kernel with scale 1 / shift 0.  Its tables are
    // indexed [b * C + channel] with C = x.C, and the identity tables hold 512 entries per sample: refill per C is not needed
    // because every entry is the same value.
    void gn_apply_ident(const TRef& x, const TRef& u) { gn_apply(x, ident_sc, ident_sh, u, ACT_NONE, RS_UP); }
};

// images -> moments: conv_in, four down blocks of two ResnetBlocks (128, 256, 512, 512; a stride-2 convolution after the first three), the mid block,
// GroupNorm + SiLU + conv_out, quant_conv.  The posterior is natinf_vae_encode's own last launch.
struct VaeEncBuilder : VaeBase {
    natinf_vae_enc& V;
    explicit VaeEncBuilder(natinf_vae_enc& e) : VaeBase(e), V(e) {}

    // diffusers' Downsample2D(padding = 0) after F.pad(x, (0, 1, 0, 1)): 3x3, stride 2, one zero row / column at the bottom / right.  As the `ddpm` plan's
    // emit_downconv: an im2col pass (k_inc_im2col, K order tap-major) + one GEMM, whose epilogue writes the partial table the next norm1 consumes.
    TRef downconv(const TRef& x, int C, Part& yp) {
        const int rin = x.res, ro = rin / 2, Kd = 9 * C;
        const int64_t pw = take((int64_t)C * C * 9), pb = take(C);
        const int64_t w = wres((int64_t)C * Kd * 2);
        E.packs.push_back([=](const PackCtx& p) {              // k = tap * C + c (the im2col order)
            const int64_t n = (int64_t)C * C * 9;
            hipLaunchKernelGGL(k_pack_conv, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream, p.params + pw, reinterpret_cast<bf16*>(p.packed + w), C, C, 9, Kd, 0, C, 0, 1.0f);
        });
        const int64_t b = pack_f32(pb, C);
        const int64_t col = arena.alloc((int64_t)ro * ro * Kd * 2);
        TRef y = new_act(ro, C);
        const Part pt = new_part(ro, C);
        op([=](const Ctx& c) {
            const int64_t M = (int64_t)c.B * ro * ro, total = M * (Kd / 8);
            hipLaunchKernelGGL(k_inc_im2col, dim3(grid1d(total, 256, 1 << 30)), dim3(256), 0, c.stream, c.act(x), rin, rin, x.ld, C, 3, 3, 2, 0, 0, ro, ro, Kd,
                               c.at<bf16>(col), total);
            GemmArgs g = gemm_defaults();
            g.a0 = c.at<bf16>(col); g.a0_ld = Kd; g.a0_C = Kd; g.M = (int)M; g.N = C; g.b = c.w<bf16>(w); g.b_ld = Kd; g.bias_n = c.w<float>(b);
            g.log_rows_per_sample = 2 * ilog2(ro); g.logHW = 2 * ilog2(ro); g.logW = ilog2(ro);
            g.c = c.act(y); g.c_ld = y.ld;
            if (pt.valid()) { g.gn_part = c.at<float>(pt.off); g.gn_quads = pt.quads; }
            const int bm = launch_gemm(g, c.stream);
            if (pt.valid()) c.part_bm[pt.id] = bm;
        });
        arena.release(col);
        yp = pt;
        return y;
    }

    void build() {
        const int Cl = V.Cl, r = V.r, R = 8 * r, N2 = 2 * Cl;
        // the moments' workspace copy first: at offset 0 of the arena and never released (natinf_vae_encode hands it to the posterior launch)
        V.mom_off = arena.alloc((int64_t)N2 * r * r * 4);
        // conv_in: the picture as a zero-bordered 64-channel NHWC tensor, 3x3 conv (K padded to 576) to 128
        const int64_t p_iw = take((int64_t)128 * 3 * 9), p_ib = take(128);
        const int64_t wi = wres((int64_t)128 * 576 * 2);
        E.packs.push_back([=](const PackCtx& p) {
            const int64_t n = (int64_t)128 * 576;
            hipLaunchKernelGGL(k_fill_bf16_zero, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream, reinterpret_cast<bf16*>(p.packed + wi), n);
        });
        pack_conv3(p_iw, wi, 128, 3, 576);
        const int64_t bi = pack_f32(p_ib, 128);
        TRef z = new_act(R, 64, 1);
        op([=](const Ctx& c) { launch_vae_images(c.x, c.act(z), R, c.B, c.stream); });
        TRef x = new_act(R, 128);
        Part xp = conv(z, 64, 128, wi, 576, bi, x, nullptr, 0, nullptr), np;
        arena.release(z.off);
        auto step = [&](TRef nx) { arena.release(x.off); x = nx; free_part(xp); xp = np; np = Part(); };
        const int chans[4] = {128, 256, 512, 512};
        int cin = 128;
        for (int i = 0; i < 4; ++i) {
            const int cout = chans[i];
            for (int j = 0; j < 2; ++j) step(resnet(x, xp, j == 0 ? cin : cout, cout, np));
            if (i < 3) step(downconv(x, cout, np));
            cin = cout;
        }
        step(resnet(x, xp, 512, 512, np));
        step(attention(x, xp, np));
        step(resnet(x, xp, 512, 512, np));
        // conv_norm_out + SiLU + conv_out -> fp32 NCHW moments in the workspace, quant_conv on them -> the caller's moments (c.out)
        const GNp gno = take_gn(512);
        const int64_t p_ow = take((int64_t)N2 * 512 * 9), p_ob = take(N2);
        const int64_t wo = wres((int64_t)N2 * 4608 * 2);
        pack_conv3(p_ow, wo, N2, 512, 4608);
        const int64_t bo = pack_f32(p_ob, N2);
        const int64_t p_qw = take((int64_t)N2 * N2), p_qb = take(N2);
        const int64_t wq = pack_f32(p_qw, (int64_t)N2 * N2), bq = pack_f32(p_qb, N2);
        const int64_t sc = arena.alloc((int64_t)512 * 4), sh = arena.alloc((int64_t)512 * 4);
        gn_stats(x, gno, sc, sh, xp);
        TRef u = new_act(r, 512, 1);
        gn_apply(x, sc, sh, u, ACT_SILU, RS_NONE);
        const int64_t raw = arena.alloc((int64_t)N2 * r * r * 4);
        const int logW = ilog2(r);
        op([=](const Ctx& c) {
            GemmArgs g = gemm_defaults();
            g.a0 = c.act(u); g.a0_ld = u.ld; g.a0_C = 512; g.taps = 9; g.logW = logW; g.logHW = 2 * logW; g.a0_padded = 1;
            g.M = c.B * r * r; g.N = N2; g.b = c.w<bf16>(wo); g.b_ld = 4608; g.bias_n = c.w<float>(bo);
            g.c = c.at<float>(raw); g.c_mode = OUT_F32_NCHW;
            launch_gemm(g, c.stream);
            const int64_t tot = (int64_t)c.B * N2 * r * r;
            ncsn_vq::launch(c.at<float>(raw), c.w<float>(wq), c.w<float>(bq), c.out, N2, r * r, tot, (void*)c.stream);
        });
        E.part_bm.assign(n_parts > 0 ? n_parts : 1, 128);
        finish();
    }
};

}  // namespace

extern "C" {

int natinf_vae_create(natinf_vae_t* out, int latent_ch, int latent_res) {
    if (!out || latent_ch < 1 || latent_ch > 64 || (latent_res != 8 && latent_res != 16 && latent_res != 32 && latent_res != 64 && latent_res != 128)) return NATINF_EINVAL;
    natinf_vae* e = new natinf_vae();
    e->Cl = latent_ch; e->r = latent_res;
    VaeBuilder b(*e);
    b.build();
    *out = e;
    return NATINF_OK;
}
int natinf_vae_destroy(natinf_vae_t h) { if (!h) return NATINF_EINVAL; delete h; return NATINF_OK; }
int64_t natinf_vae_param_count(natinf_vae_t h) { return h ? h->n_params : NATINF_EINVAL; }
int64_t natinf_vae_packed_bytes(natinf_vae_t h) { return h ? h->packed_bytes : NATINF_EINVAL; }
int64_t natinf_vae_workspace_bytes(natinf_vae_t h, int max_batch) { return h && max_batch > 0 ? h->ws_per_image * (int64_t)max_batch : NATINF_EINVAL; }
int natinf_vae_load(natinf_vae_t h, const float* params_f32, int64_t n_params, void* packed, int64_t packed_bytes, natinf_stream_t stream) {
    return h ? h->load(params_f32, n_params, packed, packed_bytes, (hipStream_t)stream) : NATINF_EINVAL;
}
int natinf_vae_decode(natinf_vae_t h, const float* latents, float* images, int B, void* workspace, int64_t workspace_bytes, natinf_stream_t stream) {
    if (!h) return NATINF_EINVAL;
    return h->run(latents, latents, images, B, workspace, workspace_bytes, (hipStream_t)stream);
}

int natinf_vae_enc_create(natinf_vae_enc_t* out, int latent_ch, int latent_res) {
    // (latent_res 128 -- 1024^2 images -- is the next size: include/natinf_vae.h)
    if (!out || latent_ch < 1 || latent_ch > 32 || (latent_res != 8 && latent_res != 16 && latent_res != 32 && latent_res != 64)) return NATINF_EINVAL;
    natinf_vae_enc* e = new natinf_vae_enc();
    e->Cl = latent_ch; e->r = latent_res;
    VaeEncBuilder b(*e);
    b.build();
    *out = e;
    return NATINF_OK;
}
int natinf_vae_enc_destroy(natinf_vae_enc_t h) { if (!h) return NATINF_EINVAL; delete h; return NATINF_OK; }
int64_t natinf_vae_enc_param_count(natinf_vae_enc_t h) { return h ? h->n_params : NATINF_EINVAL; }
int64_t natinf_vae_enc_packed_bytes(natinf_vae_enc_t h) { return h ? h->packed_bytes : NATINF_EINVAL; }
int64_t natinf_vae_enc_workspace_bytes(natinf_vae_enc_t h, int max_batch) { return h && max_batch > 0 ? h->ws_per_image * (int64_t)max_batch : NATINF_EINVAL; }
int natinf_vae_enc_load(natinf_vae_enc_t h, const float* params_f32, int64_t n_params, void* packed, int64_t packed_bytes, natinf_stream_t stream) {
    return h ? h->load(params_f32, n_params, packed, packed_bytes, (hipStream_t)stream) : NATINF_EINVAL;
}
int natinf_vae_encode(natinf_vae_enc_t h, const float* images, float* moments, float* latents, int B, int sample, float scale, float shift,
                      uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                      void* workspace, int64_t workspace_bytes, natinf_stream_t stream) {
    if (!h || !images || (!moments && !latents) || !workspace || B < 1) return NATINF_EINVAL;
    const int64_t hw = (int64_t)h->r * h->r;
    if (((int64_t)h->Cl * hw) % 4 || (((int64_t)h->Cl * hw / 4) >> 32)) return NATINF_EINVAL;      // the posterior's refusals, before anything is launched
    float* mom = moments ? moments : reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + h->mom_off * B);
    const int rc = h->run(images, images, mom, B, workspace, workspace_bytes, (hipStream_t)stream);
    if (rc != NATINF_OK || !latents) return rc;
    return natinf_vae_posterior_f32(mom, latents, B, h->Cl, hw, sample, scale, shift, seed, image_index, first_index, index_stride, stream);
}

// k_gn_fold alone (include/natinf_ncsnpp.h; tests/test_gpu_gn_kernels.py), with VaeBase::gn_stats' launch shape: grid (tps / fold, B).  quads must divide 256: with
// quads = 96 the threads 192..255 would form a third, partial lane beside lanes = 2 and their tiles would be added twice.  VaeBase launches quads = C / 4 in {32, 64, 128}.
int natinf_debug_gn_fold(const float* P, int tps, int quads, int fold, int B, float* out, natinf_stream_t stream) {
    if (!P || !out || B < 1 || B > 65535 || quads < 1 || quads > 256 || 256 % quads || fold < 1 || tps < fold || tps % fold) return NATINF_EINVAL;
    if ((reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(out)) % 8) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_gn_fold, dim3((unsigned)(tps / fold), (unsigned)B), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(P), tps, quads, fold,
                       reinterpret_cast<float2*>(out));
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

// The input passes and the encoder's quant_conv alone (include/natinf_vae.h; tests/test_gpu_glue_kernels.py): the plans' own launchers, so no kernel is instantiated
// for these entries.
int natinf_debug_vae_latents(const float* z, const float* W, const float* bias, void* y, int C, int r, int B, natinf_stream_t stream) {
    if (!z || !W || !bias || !y || C < 1 || C > 64 || r < 1 || r > 4096 || B < 1 || (int64_t)B * (r + 2) * (r + 2) * 64 > INT32_MAX) return NATINF_EINVAL;
    if (reinterpret_cast<uintptr_t>(y) % 2) return NATINF_EINVAL;
    launch_vae_latents(z, W, bias, (bf16*)y, C, r, B, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_debug_vae_images(const float* img, void* y, int R, int B, natinf_stream_t stream) {
    if (!img || !y || R < 1 || R > 16384 || B < 1 || (int64_t)B * (R + 2) * (R + 2) * 64 > INT32_MAX) return NATINF_EINVAL;
    if (reinterpret_cast<uintptr_t>(y) % 16) return NATINF_EINVAL;                  // a pixel's 128 bytes go out as eight 16-byte stores
    launch_vae_images(img, (bf16*)y, R, B, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_debug_vae_quant(const float* m, const float* W, const float* bias, float* out, int N, int hw, int B, natinf_stream_t stream) {
    if (!m || !W || !bias || !out || N < 1 || N > 64 || hw < 1 || B < 1 || (int64_t)B * N * hw > INT32_MAX) return NATINF_EINVAL;      // N = 2 latent_ch <= 64 (natinf_vae_enc_create)
    ncsn_vq::launch(m, W, bias, out, N, hw, (int64_t)B * N * hw, (void*)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

}  // extern "C"
