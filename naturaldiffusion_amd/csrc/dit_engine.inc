// dit_engine.inc -- DiT denoiser engine (C ABI of include/natinf_dit.h); included at the end of ncsnpp.hip: one translation
// unit with the GEMM launch layer (gemm_launch.h), the engine base (engine_core.h) and the packing kernels.  The row and glue kernels it launches
// beside the GEMMs are transformer_rows.h's, its plan is written in the recipes of transformer_plan.h; both are shared with mmdit_engine.inc.
//
// One forward = patch-embed(+pos) -> conditioning (t-MLP + label row -> SiLU) -> ONE GEMM for every block's adaLN
// modulation (6*depth+2 vectors per sample) -> depth x { LN+modulate, q|k GEMM, V^T GEMM, per-head QK^T / softmax /
// PV, proj GEMM with gate*(.)+x epilogue, LN+modulate, fc1 GEMM + GELU(tanh), fc2 GEMM with gate*(.)+x epilogue }
// -> LN+modulate -> linear -> unpatchify.  Residual stream fp32, GEMM operands bf16.
// NATINF_DIT_FP8: the q | k | v, fc1 and fc2 GEMMs of every block on e4m3 operands (include/natinf_dit.h states the arithmetic); everything else as above.
// Reference: deps/DiT/models.py:19-20,27-99,105-146,222-253,279-326.
#include "natinf_dit.h"
#include "transformer_plan.h"
#include "attn_fused.h"
#include "dit_flash.h"

struct natinf_dit : EngineCore {
    int depth = 0, D = 0, heads = 0, hd = 0, nmod = 0;
    int input_size = 32, T = 256;        // latent side S and tokens (S / 2)^2: natinf_dit_create_sized
    const int32_t* y = nullptr;          // per-forward
    bool unfused_attention = false;      // NATINF_DIT_UNFUSED_ATTENTION: per-head GEMM / softmax / GEMM (also used when head_dim > 96)
    bool fp8 = false;                    // NATINF_DIT_FP8: q | k | v, fc1 and fc2 on e4m3 operands (weights: a scale per output channel; LN-modulate rows: a scale per token; GELU(fc1): E8M0 block scales)
    bool stream16 = false;               // natinf_set_dit_stream16 (read when the plan is BUILT): the residual stream x [T][D] in IEEE half, not fp32 (as the MMDiT engine's image stream)
    // NATINF_DIT_STREAM_GUARD: EngineCore::guard_sites = 1 + 2 depth -- the patch embedding (site 0), then per block the attention-projection update (1 + 2 i) and the MLP update (2 + 2 i)
};

namespace {

constexpr int DIT_STREAM16_DEFAULT = 1;          // (round 6: DiT-XL/2 forward of 16 6.53 -> 6.28 ms; profiles/r06/dit_stream16_ab.txt)
int g_dit_stream16 = DIT_STREAM16_DEFAULT;      // natinf_set_dit_stream16

// qkv: [B*256][3 D] (q | k | v columns, one GEMM); v is transposed inside the attention kernel on its way into LDS (k_attn_fused<., ., false, true>).
// More than 256 tokens: the streaming kernel of dit_flash.h on the same buffer (launch_dit_flash).
template <int NQK, int ND>
void launch_attn(const bf16* qkv, bf16* o, int B, int D, int H, int hd, hipStream_t s) {
    using Cfg = AttnCfg<NQK, ND>;
    auto kern = &k_attn_fused<NQK, ND, false, true>;
    hipLaunchKernelGGL(kern, dim3((unsigned)(B * H)), dim3(Cfg::THREADS), Cfg::LDS_BYTES, s, qkv, 3 * D, D, qkv + 2 * D, o, D, H, hd,
                       1.0f / sqrtf((float)hd));
}
bool configure_dit_attention() {      // (k_attn_fused<2,4> / <3,5> / <3,6> with v as V^T: superseded by these row-major-v forms)
    return set_lds<AttnCfg<2, 4>>(&k_attn_fused<2, 4, false, true>) && set_lds<AttnCfg<3, 5>>(&k_attn_fused<3, 5, false, true>) &&
           set_lds<AttnCfg<3, 6>>(&k_attn_fused<3, 6, false, true>);
}

struct DitBuilder : TransformerBuilder {
    natinf_dit& E;
    explicit DitBuilder(natinf_dit& e) : TransformerBuilder(e), E(e) {}
    void build() {
        const int D = E.D, H = E.heads, hd = E.hd, T = E.T, depth = E.depth, gs = E.input_size / 2;       // gs: tokens per latent side
        const int log_T = T == 256 ? 8 : 10;                        // rows per sample of the gated epilogues (256 or 1,024 tokens)
        const int nmod = (6 * depth + 2) * D;
        E.nmod = nmod;
        // ---- parameters (order documented in natinf_dit.h)
        const int64_t p_pos = take((int64_t)T * D), p_pw = take((int64_t)D * 16), p_pb = take(D);
        const int64_t w_pos = pack_f32(p_pos, (int64_t)T * D), w_pw = pack_f32_transposed(p_pw, D, 16), w_pb = pack_f32(p_pb, D);
        const Lin l_t0 = linear(D, 256), l_t2 = linear(D, D);
        const int64_t p_tab = take((int64_t)1001 * D), w_tab = pack_f32(p_tab, (int64_t)1001 * D);
        const Lin l_mod{wres((int64_t)nmod * D * 2), wres((int64_t)nmod * 4)};       // all adaLN linears, stacked

        // ---- workspace (bytes per image)
        const bool fused_attn = hd <= 96 && !E.unfused_attention;
        // fused attention: q | k | v of a block are ONE GEMM into [T][3 D]; the per-head GEMM path keeps q | k and the batched V^T = W_v h^T GEMM
        const int QL = fused_attn ? 3 * D : 2 * D;
        const bool s16 = E.stream16;                                // the residual stream in IEEE half (the update stays fp32, one rounding per update)
        const int64_t x = arena.alloc((int64_t)T * D * (s16 ? 2 : 4)), h = arena.alloc((int64_t)T * D * 2), qk = arena.alloc((int64_t)T * QL * 2);
        const int64_t vT = fused_attn ? 0 : arena.alloc((int64_t)D * T * 2);
        const int64_t S = fused_attn ? 0 : arena.alloc((int64_t)H * T * T * 4), P = fused_attn ? 0 : arena.alloc((int64_t)H * T * T * 2);
        const bool fp8 = E.fp8;
        const int64_t o = arena.alloc((int64_t)T * D * 2), f = fp8 ? 0 : arena.alloc((int64_t)T * 4 * D * 2), mod = arena.alloc((int64_t)nmod * 4);
        // fp8 mode: LN-modulate rows as e4m3 + a scale per token; GELU(fc1) as e4m3 + one E8M0 scale per 32 columns, K-tile-major planes of B * T rows (ncsnpp_kernels.h).
        // Every GEMM here has M = B * T rows, a whole number of 256-row tiles, and an attention launch is one (sample, head) of exactly T rows: no kernel reads an fp8 / MX
        // operand beyond the rows the same forward wrote, so nothing has to be zeroed (the MMDiT's padded joint sequence does: mmdit_engine.inc).
        const int64_t h8 = fp8 ? arena.alloc((int64_t)T * D) : 0, sx = fp8 ? arena.alloc((int64_t)T * 4) : 0;
        const int64_t f8 = fp8 ? arena.alloc((int64_t)T * 4 * D) : 0, fmx = fp8 ? arena.alloc((int64_t)T * 4 * D / 32) : 0;
        constexpr int SK_MAX = 4;                                   // split-K slices of fc2 at small batches (launch_gemm decides: w128_splitk_slices)
        const int64_t skw = arena.alloc((int64_t)SK_MAX * T * D * 4);
        const int64_t tf = arena.alloc(256 * 2), t1 = arena.alloc((int64_t)D * 2), c0 = arena.alloc((int64_t)D * 4), cs = arena.alloc((int64_t)D * 2);
        const int64_t tok = arena.alloc((int64_t)T * 32 * 4);

        natinf_dit* eng = &E;
        op([=](const Ctx& c) {                                      // embeddings and conditioning
            const int64_t prow = (int64_t)c.B * T;
            launch_patch_embed(c.x, c.w<float>(w_pw), c.w<float>(w_pb), c.w<float>(w_pos), c.at<float>(x), 4, gs, D, prow, s16, c.site(0), c.stream);
            launch_dit_time_freq(c.labels, c.at<bf16>(tf), c.B, c.stream);
            launch_gemm(dense(c, c.at<bf16>(tf), 256, c.B, l_t0, D, ACT_SILU, c.at<bf16>(t1), OUT_BF16), c.stream);       // SiLU(Linear_0(t_freq))
            launch_gemm(dense(c, c.at<bf16>(t1), D, c.B, l_t2, D, ACT_NONE, c.at<float>(c0), OUT_F32), c.stream);        // Linear_2(.) -> fp32
            launch_dit_cond(c.at<float>(c0), c.w<float>(w_tab), eng->y, c.at<bf16>(cs), D, c.B, c.stream);
            launch_gemm(dense(c, c.at<bf16>(cs), D, c.B, l_mod, nmod, ACT_NONE, c.at<float>(mod), OUT_F32), c.stream);   // every adaLN_modulation Linear at once
        });

        auto ln_mod = [=](int shift_off, int scale_off, bool to8) {      // x -> h (bf16 rows), or to8: -> h8 + sx (e4m3 rows + per-token scales)
            return [=](const Ctx& c) {
                const float* m = c.at<float>(mod);
                const int64_t rows = (int64_t)c.B * T;
                if (to8) launch_ln_modulate<RowsFp8>(c.at<float>(x), m + shift_off, m + scale_off, nmod, c.at<uint8_t>(h8), c.at<float>(sx), D, rows, T, c.stream, s16);
                else launch_ln_modulate<RowsBf16>(c.at<float>(x), m + shift_off, m + scale_off, nmod, c.at<bf16>(h), nullptr, D, rows, T, c.stream, s16);
            };
        };
        auto update = [=](GemmArgs g, const Ctx& c, int gate_off, int site) {      // x += gate * (. + bias), g.c being x
            return gated(g, c.at<float>(mod) + gate_off, nmod, log_T, 0, c.at<float>(x), D, s16, c.site(site));
        };

        for (int i = 0; i < depth; ++i) {
            // (the checkpoint's qkv rows are q, k, v in this order)      fp8: e4m3 bytes + per-output-channel scales in place of the bf16 matrix, both matrices in front of the biases
            const int64_t p_qkvw = take((int64_t)3 * D * D), p_qkvb = take(3 * D), p_vw = p_qkvw + (int64_t)2 * D * D, p_vb = p_qkvb + 2 * D;
            Lin l_qk{0, 0}, l_v{0, 0}, l_f1{0, 0}, l_f2{0, 0};
            Lin8 l_qk8{0, 0, 0}, l_v8{0, 0, 0}, l_f18{0, 0, 0}, l_f28{0, 0, 0};
            if (fp8) {
                l_qk8 = weights8(p_qkvw, QL, D);
                if (!fused_attn) l_v8 = weights8(p_vw, D, D);
                l_qk8.b = pack_f32(p_qkvb, QL);
                if (!fused_attn) l_v8.b = pack_f32(p_vb, D);
            } else {
                l_qk = packed(p_qkvw, p_qkvb, QL, D);
                if (!fused_attn) l_v = packed(p_vw, p_vb, D, D);
            }
            const Lin l_pr = linear(D, D);
            if (fp8) { l_f18 = linear8(4 * D, D); l_f28 = linear8(D, 4 * D); }
            else { l_f1 = linear(4 * D, D); l_f2 = linear(D, 4 * D); }
            const int m0 = i * 6 * D;                                // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
            linear_at(6 * D, D, l_mod.w + (int64_t)m0 * D * 2, l_mod.b + (int64_t)m0 * 4);

            op(ln_mod(m0, m0 + D, fp8));
            op([=](const Ctx& c) {
                const int M = c.B * T;
                if (fp8) {                                          // q | k (| v)      (bf16 out in both modes: the attention stays bf16)
                    GemmArgs g = dense(c, nullptr, D, M, l_qk8, QL, ACT_NONE, c.at<bf16>(qk), OUT_BF16);
                    a_fp8_rows(g, c.at<uint8_t>(h8), c.at<float>(sx));
                    launch_gemm_fp8(g, c.stream);
                } else launch_gemm(dense(c, c.at<bf16>(h), D, M, l_qk, QL, ACT_NONE, c.at<bf16>(qk), OUT_BF16), c.stream);
                if (fused_attn && T != 256) {                       // keys streamed through LDS (dit_flash.h)
                    const bf16* qkv = c.at<bf16>(qk);
                    launch_dit_flash(qkv, qkv + D, qkv + 2 * D, 3 * D, c.at<bf16>(o), D, c.B, H, T, hd, c.stream);
                } else if (fused_attn) {                            // softmax(q k^T / sqrt(hd)) v, all heads, one launch
                    if (hd <= 64) launch_attn<2, 4>(c.at<bf16>(qk), c.at<bf16>(o), c.B, D, H, hd, c.stream);
                    else if (hd <= 80) launch_attn<3, 5>(c.at<bf16>(qk), c.at<bf16>(o), c.B, D, H, hd, c.stream);
                    else launch_attn<3, 6>(c.at<bf16>(qk), c.at<bf16>(o), c.B, D, H, hd, c.stream);
                } else {
                    // V^T[b] = Wv h[b]^T + bv  ([D][T] per sample)
                    if (fp8) launch_gemm_fp8(vt8(c, l_v8, D, c.at<uint8_t>(h8), c.at<float>(sx), T, c.at<bf16>(vT), T), c.stream);
                    else launch_gemm(vt(c, l_v, D, c.at<bf16>(h), T, c.at<bf16>(vT), T), c.stream);
                    for (int hh = 0; hh < H; ++hh) {                // S[b][hh] = q k^T / sqrt(hd)
                        GemmArgs g = gemm_defaults();
                        g.a0 = c.at<bf16>(qk) + hh * hd; g.a0_ld = 2 * D; g.a0_C = hd; g.a_bs = (int64_t)T * 2 * D; g.M = T; g.N = T;
                        g.b = c.at<bf16>(qk) + D + hh * hd; g.b_ld = 2 * D; g.b_bs = (int64_t)T * 2 * D;
                        g.scale = 1.0f / sqrtf((float)hd);
                        g.c = c.at<float>(S) + (int64_t)hh * T * T; g.c_ld = T; g.c_bs = (int64_t)H * T * T; g.c_mode = OUT_F32; g.batch = c.B;
                        launch_gemm(g, c.stream);
                    }
                    const int64_t rows = (int64_t)c.B * H * T;
                    if (T == 256) hipLaunchKernelGGL(k_softmax_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, c.stream, c.at<float>(S), c.at<bf16>(P), T, rows);
                    else hipLaunchKernelGGL(k_softmax_rows_1k, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, c.stream, c.at<float>(S), c.at<bf16>(P), T, rows);
                    for (int hh = 0; hh < H; ++hh) {                // o[b][:, hh*hd : (hh+1)*hd] = P V
                        GemmArgs g = gemm_defaults();
                        g.a0 = c.at<bf16>(P) + (int64_t)hh * T * T; g.a0_ld = T; g.a0_C = T; g.a_bs = (int64_t)H * T * T; g.M = T; g.N = hd;
                        g.b = c.at<bf16>(vT) + (int64_t)hh * hd * T; g.b_ld = T; g.b_bs = (int64_t)D * T;
                        g.c = c.at<bf16>(o) + hh * hd; g.c_ld = D; g.c_bs = (int64_t)T * D; g.batch = c.B;
                        launch_gemm(g, c.stream);
                    }
                }
                // x += gate_msa * (o Wproj + b)
                launch_gemm(update(dense(c, c.at<bf16>(o), D, M, l_pr, D, ACT_NONE, c.at<float>(x), OUT_F32), c, m0 + 2 * D, 1 + 2 * i), c.stream);
            });
            op(ln_mod(m0 + 3 * D, m0 + 4 * D, fp8));
            op([=](const Ctx& c) {
                const int M = c.B * T;
                if (fp8) {
                    GemmArgs g = dense(c, nullptr, D, M, l_f18, 4 * D, ACT_GELU_TANH, c.at<uint8_t>(f8), OUT_FP8_MX);      // GELU_tanh(fc1) -> e4m3 + a scale per 32 columns: fc2's operand
                    a_fp8_rows(g, c.at<uint8_t>(h8), c.at<float>(sx));
                    g.c_mx = c.at<uint8_t>(fmx); g.c_mx_ld = M;
                    launch_gemm_fp8(g, c.stream);
                    g = update(dense(c, nullptr, 4 * D, M, l_f28, D, ACT_NONE, c.at<float>(x), OUT_F32), c, m0 + 5 * D, 2 + 2 * i);      // x += gate_mlp * (f8 W2^T + b)
                    a_fp8_mx(g, c.at<uint8_t>(f8), c.at<uint8_t>(fmx), M);
                    launch_gemm_fp8(g, c.stream);
                } else {
                    launch_gemm(dense(c, c.at<bf16>(h), D, M, l_f1, 4 * D, ACT_GELU_TANH, c.at<bf16>(f), OUT_BF16), c.stream);      // GELU_tanh(fc1)
                    GemmArgs g = update(dense(c, c.at<bf16>(f), 4 * D, M, l_f2, D, ACT_NONE, c.at<float>(x), OUT_F32), c, m0 + 5 * D, 2 + 2 * i);      // x += gate_mlp * fc2
                    g.splitk_ws = c.at<float>(skw); g.splitk_max = SK_MAX;
                    launch_gemm(g, c.stream);
                }
            });
        }
        // ---- final layer
        const Lin l_fin = linear(32, D);
        const int mf = 6 * depth * D;
        linear_at(2 * D, D, l_mod.w + (int64_t)mf * D * 2, l_mod.b + (int64_t)mf * 4);
        op(ln_mod(mf, mf + D, false));
        op([=](const Ctx& c) {
            launch_gemm(dense(c, c.at<bf16>(h), D, c.B * T, l_fin, 32, ACT_NONE, c.at<float>(tok), OUT_F32), c.stream);
            launch_unpatchify(c.at<float>(tok), c.out, 8, gs, c.B, c.stream);
        });
        finish();
    }
};

}  // namespace

extern "C" {

int natinf_dit_create(natinf_dit_t* out, int depth, int hidden, int heads, int flags) {
    return natinf_dit_create_sized(out, depth, hidden, heads, 32, flags);
}
int natinf_dit_create_sized(natinf_dit_t* out, int depth, int hidden, int heads, int input_size, int flags) {
    if (!out || (flags & ~(NATINF_DIT_UNFUSED_ATTENTION | NATINF_DIT_FP8 | NATINF_DIT_STREAM_GUARD)) || ((flags & NATINF_DIT_FP8) && hidden % 128) || depth <= 0 || hidden <= 0 || heads <= 0 || hidden % 64 || hidden % heads || (hidden / heads) % 8 || hidden > 1536)
        return NATINF_EINVAL;
    if (input_size != 32 && input_size != 64) return NATINF_EINVAL;
    natinf_dit* e = new natinf_dit();
    e->depth = depth; e->D = hidden; e->heads = heads; e->hd = hidden / heads;
    e->input_size = input_size; e->T = (input_size / 2) * (input_size / 2);
    e->unfused_attention = (flags & NATINF_DIT_UNFUSED_ATTENTION) != 0;
    e->fp8 = (flags & NATINF_DIT_FP8) != 0;
    e->stream16 = g_dit_stream16 != 0;
    e->guard_sites = (flags & NATINF_DIT_STREAM_GUARD) ? 1 + 2 * depth : 0;
    DitBuilder b(*e);
    b.build();
    *out = e;
    return NATINF_OK;
}
int natinf_set_dit_stream16(int on) { g_dit_stream16 = on < 0 ? DIT_STREAM16_DEFAULT : (on != 0); return NATINF_OK; }
int natinf_dit_input_size(natinf_dit_t h) { return h ? h->input_size : NATINF_EINVAL; }
int natinf_dit_destroy(natinf_dit_t h) { if (!h) return NATINF_EINVAL; delete h; return NATINF_OK; }
int64_t natinf_dit_param_count(natinf_dit_t h) { return h ? h->n_params : NATINF_EINVAL; }
int64_t natinf_dit_packed_bytes(natinf_dit_t h) { return h ? h->packed_bytes : NATINF_EINVAL; }
int64_t natinf_dit_workspace_bytes(natinf_dit_t h, int max_batch) { return h && max_batch > 0 ? h->workspace_bytes(max_batch) : NATINF_EINVAL; }
int natinf_dit_stream_sites(natinf_dit_t h) { return h && h->guard_sites ? h->guard_sites : NATINF_EINVAL; }
int natinf_dit_stream_status_reset(natinf_dit_t h, void* workspace, natinf_stream_t stream) { return h ? h->status_reset(workspace, (hipStream_t)stream) : NATINF_EINVAL; }
int natinf_dit_stream_status(natinf_dit_t h, const void* workspace, uint32_t* out_dev, natinf_stream_t stream) { return h ? h->status_read(workspace, out_dev, (hipStream_t)stream) : NATINF_EINVAL; }

int natinf_dit_load(natinf_dit_t h, const float* params_f32, int64_t n_params, void* packed, int64_t packed_bytes, natinf_stream_t stream) {
    return h ? h->load(params_f32, n_params, packed, packed_bytes, (hipStream_t)stream) : NATINF_EINVAL;
}

int natinf_dit_forward(natinf_dit_t h, const float* z, const float* t, const int32_t* y, float* out, int B, void* workspace,
                       int64_t workspace_bytes, natinf_stream_t stream) {
    if (!h || !y) return NATINF_EINVAL;
    h->y = y;
    return h->run(z, t, out, B, workspace, workspace_bytes, (hipStream_t)stream);
}

int natinf_dit_attention_bf16(const void* q, const void* k, const void* v, int ld, void* o, int ld_o, int B, int T, int H, int hd, int flags,
                              natinf_stream_t stream) {
    if (!q || !k || !v || !o || B <= 0 || H <= 0 || hd < 8 || hd > 96 || hd % 8 || ld % 8 || ld < H * hd || ld_o % 4 || ld_o < H * hd) return NATINF_EINVAL;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) % 16 || reinterpret_cast<uintptr_t>(o) % 8) return NATINF_EINVAL;
    if (flags & ~NATINF_DIT_ATTN_RESIDENT) return NATINF_EINVAL;
    const bool resident = (flags & NATINF_DIT_ATTN_RESIDENT) != 0;
    if (resident ? T != 256 : (T < 256 || T > 4096 || T % 128)) return NATINF_EINVAL;
    if (!configure_gemm_kernels()) return NATINF_ENODEV;
    if (resident) {                                      // k_attn_fused addresses k as q + k_off
        const int64_t k_off = (int64_t)(reinterpret_cast<intptr_t>(k) - reinterpret_cast<intptr_t>(q)) / 2;
        if (k_off > INT32_MAX || k_off < INT32_MIN) return NATINF_EINVAL;
        const bf16* qb = (const bf16*)q;
        const bf16* vb = (const bf16*)v;
        bf16* ob = (bf16*)o;
        const float sc = 1.0f / sqrtf((float)hd);
        const hipStream_t s = (hipStream_t)stream;
        auto run = [&](auto kern, int lds) { hipLaunchKernelGGL(kern, dim3((unsigned)(B * H)), dim3(512), lds, s, qb, ld, (int)k_off, vb, ob, ld_o, H, hd, sc); };
        if (hd <= 64) run(&k_attn_fused<2, 4, false, true>, AttnCfg<2, 4>::LDS_BYTES);
        else if (hd <= 80) run(&k_attn_fused<3, 5, false, true>, AttnCfg<3, 5>::LDS_BYTES);
        else run(&k_attn_fused<3, 6, false, true>, AttnCfg<3, 6>::LDS_BYTES);
    } else {
        launch_dit_flash((const bf16*)q, (const bf16*)k, (const bf16*)v, ld, (bf16*)o, ld_o, B, H, T, hd, (hipStream_t)stream);
    }
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

// The LayerNorm-modulate kernels of transformer_rows.h alone (include/natinf_dit.h; tests/test_gpu_row_kernels.py): nothing but the engines' own launcher, so no kernel
// is instantiated for this entry.  (That header cannot hold a C entry itself: stream_guard.hip includes it into an anonymous namespace.)
int natinf_debug_ln_modulate(const void* x, int x_f16, const float* shift, const float* scale, int mod_ld, void* h_bf16, void* h_fp8, float* row_scale,
                             int D, int64_t rows, int rows_per_sample, int* form_out, natinf_stream_t stream) {
    const bool to_bf16 = h_bf16 != nullptr, to_fp8 = h_fp8 != nullptr || row_scale != nullptr;
    if (!x || !shift || !scale || !form_out || to_bf16 == to_fp8 || (to_fp8 && (!h_fp8 || !row_scale))) return NATINF_EINVAL;
    if (D <= 0 || D > 1536 || D % (to_fp8 ? 128 : 64) || rows <= 0 || rows_per_sample <= 0 || mod_ld < D) return NATINF_EINVAL;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(to_bf16 ? h_bf16 : h_fp8)) % 16) return NATINF_EINVAL;
    if (to_bf16) *form_out = launch_ln_modulate<RowsBf16>((const float*)x, shift, scale, mod_ld, (bf16*)h_bf16, nullptr, D, rows, rows_per_sample, (hipStream_t)stream, x_f16 != 0);
    else *form_out = launch_ln_modulate<RowsFp8>((const float*)x, shift, scale, mod_ld, (uint8_t*)h_fp8, row_scale, D, rows, rows_per_sample, (hipStream_t)stream, x_f16 != 0);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

// The glue kernels at the two ends of the transformer engines alone (include/natinf_dit.h; tests/test_gpu_glue_kernels.py): the plans' own launchers of
// transformer_plan.h / engine_core.h on caller-supplied buffers, so no kernel is instantiated for these entries.  Every refusal comes before the first launch.
int natinf_debug_patch_embed(const float* z, const float* w, float* wt, const float* bias, const float* pos, void* x, int x_f16, uint32_t* guard,
                             int C, int g, int D, int B, natinf_stream_t stream) {
    if (!z || !w || !wt || !bias || !pos || !x || C < 1 || C > 16 || g < 1 || g > 256 || D < 64 || D > 1536 || D % 64 || B < 1) return NATINF_EINVAL;
    const int64_t rows = (int64_t)B * g * g;
    if ((rows + PE_TOK - 1) / PE_TOK > 65535 || reinterpret_cast<uintptr_t>(x) % (x_f16 ? 2 : 4) || reinterpret_cast<uintptr_t>(guard) % 4) return NATINF_EINVAL;      // grid.y
    launch_transpose_f32(w, wt, D, C * 4, (hipStream_t)stream);                      // [D][C*4] -> [C*4][D], as pack_f32_transposed at load time
    launch_patch_embed(z, wt, bias, pos, (float*)x, C, g, D, rows, x_f16 != 0, guard, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_debug_dit_time_freq(const float* t, void* emb, int B, natinf_stream_t stream) {
    if (!t || !emb || B < 1 || B > (1 << 22)) return NATINF_EINVAL;                 // i = b * 256 + j is an int in the kernel
    launch_dit_time_freq(t, (bf16*)emb, B, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_debug_dit_cond(const float* c0, const float* table, const int32_t* y, void* cs, int D, int B, natinf_stream_t stream) {
    if (!c0 || !table || !y || !cs || D < 1 || B < 1 || (int64_t)B * D > INT32_MAX) return NATINF_EINVAL;
    launch_dit_cond(c0, table, y, (bf16*)cs, D, B, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_debug_silu_bf16(const float* c, void* cs, int64_t n, natinf_stream_t stream) {
    if (!c || !cs || n < 1 || n > INT32_MAX) return NATINF_EINVAL;
    launch_silu_bf16(c, (bf16*)cs, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_debug_f32_to_bf16(const float* src, void* dst, int64_t n, natinf_stream_t stream) {
    if (!src || !dst || n < 1 || n > INT32_MAX) return NATINF_EINVAL;
    launch_f32_to_bf16(src, (bf16*)dst, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_debug_unpatchify(const float* tok, float* out, int OC, int g, int n_images, natinf_stream_t stream) {
    if (!tok || !out || OC < 1 || OC > 4096 || g < 1 || g > 4096 || n_images < 1 || (int64_t)n_images * OC * 4 * g * g > INT32_MAX) return NATINF_EINVAL;
    launch_unpatchify(tok, out, OC, g, n_images, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

}  // extern "C"
