// transformer_plan.h -- what the transformer plans (DitBuilder: dit_engine.inc, MMDitBuilder: mmdit_engine.inc) are written in: a Linear's place in the packed image
// (Lin / Lin8), the builder base that takes and packs one, and the GEMM recipes -- each fills a GemmArgs for launch_gemm / launch_gemm_fp8 (gemm_launch.h); a call site
// adds only the fields special to it.  The VAE's mid-block attention (vae_engine.inc) uses the recipes too.  The kernels beside the GEMMs: transformer_rows.h.
#pragma once
#include "engine_core.h"
#include "transformer_rows.h"

namespace {

// the patch embedding of a plan: plain or guarded (guard: the site's slot; k_patch_embed<., true>: stream_guard.hip), onto an fp32 or a half stream
inline void launch_patch_embed(const float* z, const float* Wt, const float* bias, const float* pos, float* x, int C, int g, int D, int64_t rows, bool x_f16, uint32_t* guard, hipStream_t s)
{
    if (guard) ncsn_sg::launch_patch_embed(z, Wt, bias, pos, x, C, g, D, rows, x_f16, guard, (void*)s);
    else launch_patch_embed_as<false>(z, Wt, bias, pos, x, C, g, D, rows, x_f16, nullptr, s);
}

// the glue kernels of transformer_rows.h with the grid a plan gives them: one thread per element, 256 per block.  The plans and the natinf_debug_* entries of
// dit_engine.inc (tests/test_gpu_glue_kernels.py) launch them through these and through nothing else.
inline void launch_dit_time_freq(const float* t, bf16* emb, int B, hipStream_t s)
{
    hipLaunchKernelGGL(k_dit_time_freq, dim3(grid1d((int64_t)B * 256, 256, 1 << 30)), dim3(256), 0, s, t, emb, B);
}
inline void launch_dit_cond(const float* c0, const float* table, const int32_t* y, bf16* cs, int D, int B, hipStream_t s)
{
    hipLaunchKernelGGL(k_dit_cond, dim3(grid1d((int64_t)B * D, 256, 1 << 30)), dim3(256), 0, s, c0, table, y, cs, D, B);
}
inline void launch_silu_bf16(const float* c, bf16* cs, int64_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_silu_bf16, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, s, c, cs, n);
}
inline void launch_f32_to_bf16(const float* src, bf16* dst, int64_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_f32_to_bf16, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, s, src, dst, n);
}
inline void launch_unpatchify(const float* tok, float* out, int OC, int g, int64_t n_images, hipStream_t s)       // tok [n_images * g * g][4 OC] -> out [n_images][OC][2g][2g]
{
    const int64_t tot = n_images * OC * (2 * g) * (2 * g);
    hipLaunchKernelGGL(k_unpatchify, dim3(grid1d(tot, 256, 1 << 30)), dim3(256), 0, s, tok, out, OC, g, tot);
}

struct Lin { int64_t w, b; };                                     // bf16 [out][in], fp32 bias: offsets into the packed image
struct Lin8 { int64_t w, s, b; };                                  // e4m3 bytes [out][in], per-output-channel scale, fp32 bias

struct TransformerBuilder : PlanBuilder {
    using PlanBuilder::PlanBuilder;
    Lin packed(int64_t pw, int64_t pb, int out, int in) { return Lin{pack_bf16(pw, out, in), pack_f32(pb, out)}; }      // a Linear whose parameters are already taken
    Lin8 weights8(int64_t pw, int out, int in) {                   // the matrix alone (b = 0: the caller packs the bias where the image has it)
        const Lin8 r{wres((int64_t)out * in), wres((int64_t)out * 4), 0};
        pack_fp8_at(pw, out, in, r.w, r.s);
        return r;
    }
    Lin linear(int out, int in) {                                  // takes weight then bias from the parameter stream
        const int64_t pw = take((int64_t)out * in), pb = take(out);
        return packed(pw, pb, out, in);
    }
    Lin8 linear8(int out, int in) {
        const int64_t pw = take((int64_t)out * in), pb = take(out);
        const Lin8 r{wres((int64_t)out * in), wres((int64_t)out * 4), pack_f32(pb, out)};
        pack_fp8_at(pw, out, in, r.w, r.s);
        return r;
    }
    void linear_at(int out, int in, int64_t wdst, int64_t bdst) {
        const int64_t pw = take((int64_t)out * in), pb = take(out);
        pack_bf16_at(pw, out, in, wdst);
        pack_f32_at(pb, out, bdst);
    }
};

// ---- GEMM recipes.  e4m3 operands travel through GemmArgs' bf16 pointers; every fp8 setter also sets the operand's dequantisation scales.
inline const bf16* e4m3(const uint8_t* p) { return reinterpret_cast<const bf16*>(p); }
inline void set_b(GemmArgs& g, const Ctx& c, const Lin& w) { g.b = c.w<bf16>(w.w); g.bias_n = c.w<float>(w.b); }
inline void set_b(GemmArgs& g, const Ctx& c, const Lin8& w) { g.b = e4m3(c.w<uint8_t>(w.w)); g.deq_n = c.w<float>(w.s); g.bias_n = c.w<float>(w.b); }
// A = e4m3 rows + one scale per row (the LayerNorm-modulate kernels' RowsFp8); scale_bs: rows per batch index
inline void a_fp8_rows(GemmArgs& g, const uint8_t* a8, const float* row_scale, int64_t scale_bs = 0) { g.a0 = e4m3(a8); g.deq_m = row_scale; g.deq_m_bs = scale_bs; }
// A = e4m3 + E8M0 block scales in K-tile-major planes of mx_ld rows (an OUT_FP8_MX epilogue's output, or the fp8-output attention's)
inline void a_fp8_mx(GemmArgs& g, const uint8_t* a8, const uint8_t* mx, int mx_ld, int64_t mx_bs = 0) { g.a0 = e4m3(a8); g.a_mx = mx; g.a_mx_ld = mx_ld; g.a_mx_bs = mx_bs; }

// out [M][N] = act(a [M][K] w^T + bias): the flat GEMM.  W: Lin or Lin8 (then a is set by one of the setters above)
template <class W>
GemmArgs dense(const Ctx& c, const bf16* a, int K, int M, const W& w, int N, int act, void* out, int mode)
{
    GemmArgs g = gemm_defaults();
    g.a0 = a; g.a0_ld = K; g.a0_C = K; g.M = M; g.N = N; g.b_ld = K; set_b(g, c, w);
    g.act = act; g.c = out; g.c_ld = N; g.c_mode = mode;
    return g;
}
// per-sequence batched GEMM: rows of stream `a` (T rows per sequence) -> rows of the per-sequence output
template <class W>
GemmArgs seq_gemm(const Ctx& c, const bf16* a, int K, int64_t a_bs, int T, const W& w, int N, void* out, int ld, int64_t c_bs, int mode)
{
    GemmArgs g = gemm_defaults();
    g.a0 = a; g.a0_ld = K; g.a0_C = K; g.a_bs = a_bs; g.M = T; g.N = N; g.b_ld = K; set_b(g, c, w);
    g.c = out; g.c_ld = ld; g.c_bs = c_bs; g.c_mode = mode; g.batch = c.B;
    return g;
}
// V^T[b][:, col : col + T] = Wv h[b]^T + bv, the swapped GEMM (the weights [D][D] as the row operand, keys contiguous): vT is [D][ld] per sequence
inline GemmArgs vt(const Ctx& c, const Lin& w, int D, const bf16* h, int T, bf16* vT, int ld, int col = 0)
{
    GemmArgs g = gemm_defaults();
    g.a0 = c.w<bf16>(w.w); g.a0_ld = D; g.a0_C = D; g.a_bs = 0; g.M = D; g.N = T;
    g.b = h; g.b_ld = D; g.b_bs = (int64_t)T * D; g.bias_m = c.w<float>(w.b);
    g.c = vT + col; g.c_ld = ld; g.c_bs = (int64_t)D * ld; g.batch = c.B;
    return g;
}
// ... on e4m3 operands: the weights' scales per row, the tokens' (h8 rows, row_scale) per column
inline GemmArgs vt8(const Ctx& c, const Lin8& w, int D, const uint8_t* h8, const float* row_scale, int T, bf16* vT, int ld, int col = 0)
{
    GemmArgs g = vt(c, Lin{0, w.b}, D, e4m3(h8), T, vT, ld, col);
    a_fp8_rows(g, c.w<uint8_t>(w.w), c.w<float>(w.s), 0);
    g.deq_n = row_scale; g.deq_n_bs = T;
    return g;
}
// stream += gate[sample] * (g's product + bias): the gated update of a residual stream, g.c being that stream.  The sample of row m of batch index z is
// (m >> log_rows) + z * z_samples (DiT: flat rows, log2 T and 0; MMDiT: one sequence per batch index, 30 and 1); f16: the stream is IEEE half; guard: the site's slot or null
inline GemmArgs gated(GemmArgs g, const float* gate, int gate_ld, int log_rows, int z_samples, const float* stream, int stream_ld, bool f16, uint32_t* guard)
{
    g.gate = gate; g.gate_ld = gate_ld; g.log_rows_per_sample = log_rows; g.z_samples = z_samples;
    g.resid_f32 = stream; g.resid_f32_ld = stream_ld; g.stream_f16 = f16; g.stream_guard = guard;
    return g;
}

}  // namespace
