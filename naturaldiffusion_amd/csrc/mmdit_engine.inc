// mmdit_engine.inc -- SD3 MMDiT denoiser engine (C ABI of include/natinf_mmdit.h); included after dit_engine.inc, on which it does not depend: the row and glue
// kernels it shares with the DiT engine are transformer_rows.h's, the plan base and the GEMM recipes transformer_plan.h's.
//
// Two residual streams (image tokens x [Tx][D]: fp32, or IEEE half with natinf_set_mmdit_stream16; text tokens e [Tc][D]: fp32) and one joint bf16 attention buffer per
// sequence, padded to Tp = roundup(Tx + Tc, 128) rows: Q|K [Tp][2D], V^T [D][Tp], O [Tp][D].  Per block:
//   LN+modulate both streams -> q|k GEMMs (stream-specific weights, written into the joint buffer at rows [0,Tx) and
//   [Tx,Tx+Tc)) -> V^T by the swapped GEMM (keys contiguous) -> k_flash_attn64 over the joint sequence -> per-stream
//   output projections with the gated-residual epilogue -> per-stream LN+modulate, fc1 + GELU(tanh), fc2 gated residual.
// All adaLN linears of the network run as one GEMM per forward.  include/natinf_mmdit.h states what this replaces
// and the parity status of that third-party arithmetic.
#include "natinf_mmdit.h"
#include "transformer_plan.h"
#include "flash_attn.h"

struct natinf_mmdit : EngineCore {
    int L = 0, H = 0, D = 0, Jd = 0, Pd = 0, C = 0, g = 0, Tx = 0, Tc = 0, Tp = 0, nmod = 0;
    bool fp8 = false;                    // NATINF_MMDIT_FP8: image-stream q|k, v and fc1 GEMMs on e4m3 operands
    bool stream16 = false;               // natinf_set_mmdit_stream16 (read when the plan is BUILT): the image tokens' residual stream x is IEEE half, not fp32
    const float* text = nullptr; const float* pooled = nullptr;      // per-forward
    // the text stream's launches on a HIP stream of their own (natinf_set_mmdit_text_stream): created at the first forward that wants it
    hipStream_t aux = nullptr;
    std::vector<hipEvent_t> ev;          // [0] fork, [1 + 2 i] text q | k | v of block i written, [2 + 2 i] attention of block i done, [2 L + 1] join
    bool ensure_aux() {
        if (aux) return true;
        // (the highest stream priority for it was measured too -- the image stream waits for the short text chain in front of every attention --: 55.7-55.8 ms per fp8
        // forward against 55.6-55.7, 69.1-69.4 against 69.4-69.5 bf16: nothing)
        if (hipStreamCreateWithFlags(&aux, hipStreamNonBlocking) != hipSuccess) { aux = nullptr; (void)hipGetLastError(); return false; }
        ev.assign((size_t)2 * L + 2, nullptr);
        for (auto& e : ev)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); release_aux(); return false; }
        return true;
    }
    void release_aux() {
        for (auto e : ev) if (e) (void)hipEventDestroy(e);
        ev.clear();
        if (aux) (void)hipStreamDestroy(aux);
        aux = nullptr;
    }
    ~natinf_mmdit() { release_aux(); }
};

namespace {

// natinf_attention_profile(1): every k_flash_attn64 launch -- inside an engine forward or through natinf_attention_hd64_bf16 -- is bracketed
// by a HIP event pair on ITS stream, so bench.py can quote the kernel's duration where it actually runs (between the GEMMs of a block),
// not only in an isolated back-to-back loop (the two differ by 15-25 % on this power-capped part: profiles/README.md)
struct FlashProf { bool on = false; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev, pool; } g_flash_prof;
constexpr int MMDIT_STREAM16_DEFAULT = 1;      // (round 6: -3.3 % bf16 / -5.2 % fp8 per forward of 8 sequences; 1.5e-3 / 6.6e-3 of the 28-step latents against the fp32 stream: profiles/r06/stream16_*)
int g_mmdit_stream16 = MMDIT_STREAM16_DEFAULT;      // natinf_set_mmdit_stream16 (read when a plan is BUILT): 1 = the image stream x [Tx][D] is kept in IEEE half -- the reference's SD3 pipeline is fp16
                                   // (src/SD3NaturalInference.py:175-176) -- so that the projection / fc2 epilogues and the LayerNorm-modulate passes move half the bytes; the text stream (333 tokens) stays fp32
int g_mmdit_text_flat = 1;         // natinf_set_mmdit_text_flat: the text stream's fc1 as ONE GEMM over all sequences' rows (1) or batched per sequence (0: A/B runs)
int g_mmdit_text_stream = 1;       // natinf_set_mmdit_text_stream: 1 = the text stream's launches of a block (M = 333 rows per sequence: 150 GFLOP per block at under a sixth of the chip's
                                   // rate when they run alone) go to a second HIP stream and join the image stream at the joint attention; 0 = one stream, one launch after the other
int g_flash_mode = 3;              // natinf_set_flash_mode: 0 = k_flash_attn64, 3 = k_flash_attn64_v2<1, 64> (deferred re-referencing, scores leave the MFMA as exponents, row sums on the matrix pipe, 64-key tiles: 128 registers and 32 KiB of LDS per block, three to four waves per SIMD); default 3; 1 / 2: retired
bool configure_flash_attention() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_flash_attn64), hipFuncAttributeMaxDynamicSharedMemorySize, FA_LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&k_flash_attn64_v2<1, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, FA_LDS_BYTES / 2) == hipSuccess;
}
void launch_flash(const bf16* q, const bf16* k, int ld_qk, int64_t qk_bs, const bf16* vT, bf16* o, int ld_o, int64_t o_bs, int B, int H,
                  int Tp, int T, float scale, hipStream_t s, uint8_t* o8 = nullptr, uint8_t* omx = nullptr) {
    FlashArgs a{q, k, ld_qk, qk_bs, vT, (int64_t)H * 64 * Tp, o, ld_o, o_bs, H, Tp, T, scale * 1.4426950408889634f, o8, omx};
    std::pair<hipEvent_t, hipEvent_t> e{nullptr, nullptr};
    if (g_flash_prof.on) {
        if (!g_flash_prof.pool.empty()) { e = g_flash_prof.pool.back(); g_flash_prof.pool.pop_back(); }
        else if (hipEventCreate(&e.first) != hipSuccess || hipEventCreate(&e.second) != hipSuccess) e = {nullptr, nullptr};
        if (e.first) (void)hipEventRecord(e.first, s);
    }
    const dim3 grid((unsigned)(B * H * (Tp / FA_QB)));
    if (g_flash_mode == 3) hipLaunchKernelGGL((k_flash_attn64_v2<1, 64>), grid, dim3(256), FA_LDS_BYTES / 2, s, a);
    else hipLaunchKernelGGL(k_flash_attn64, grid, dim3(256), FA_LDS_BYTES, s, a);
    if (e.first) { (void)hipEventRecord(e.second, s); g_flash_prof.ev.push_back(e); }
}

struct MMDitBuilder : TransformerBuilder {
    natinf_mmdit& E;
    explicit MMDitBuilder(natinf_mmdit& e) : TransformerBuilder(e), E(e) {}

    void build() {
        const int L = E.L, H = E.H, D = E.D, Jd = E.Jd, Pd = E.Pd, C = E.C, gr = E.g, Tx = E.Tx, Tc = E.Tc, Tp = E.Tp;
        const int nmod = (12 * (L - 1) + 8 + 2) * D;               // blocks: x 6D + text 6D (last block: 2D), norm_out 2D
        E.nmod = nmod;
        natinf_mmdit* eng = &E;
        // ---- parameters
        const int64_t p_pos = take((int64_t)Tx * D), p_pw = take((int64_t)D * C * 4), p_pb = take(D);
        const int64_t w_pos = pack_f32(p_pos, (int64_t)Tx * D), w_pw = pack_f32_transposed(p_pw, D, C * 4), w_pb = pack_f32(p_pb, D);
        const Lin t1 = linear(D, 256), t2 = linear(D, D), x1 = linear(D, Pd), x2 = linear(D, D), ce = linear(D, Jd);
        const int64_t w_mod = wres((int64_t)nmod * D * 2), b_mod = wres((int64_t)nmod * 4);

        // ---- workspace (bytes per sequence)
        const bool s16 = E.stream16;                                  // the image stream in IEEE half
        const int64_t x = arena.alloc((int64_t)Tx * D * (s16 ? 2 : 4)), e = arena.alloc((int64_t)Tc * D * 4);
        const int64_t hx = arena.alloc((int64_t)Tx * D * 2), he = arena.alloc((int64_t)Tc * D * 2);
        const int64_t qk = arena.alloc((int64_t)Tp * 2 * D * 2), vT = arena.alloc((int64_t)D * Tp * 2), o = arena.alloc((int64_t)Tp * D * 2);
        const int64_t fx = arena.alloc((int64_t)Tx * 4 * D * 2), fe = arena.alloc((int64_t)Tc * 4 * D * 2);
        const int64_t mod = arena.alloc((int64_t)nmod * 4), tf = arena.alloc(512), a1 = arena.alloc((int64_t)D * 2), a2 = arena.alloc((int64_t)D * 2);
        const int64_t pl = arena.alloc((int64_t)Pd * 2), cf = arena.alloc((int64_t)D * 4), cs = arena.alloc((int64_t)D * 2);
        const int64_t tx = arena.alloc((int64_t)Tc * Jd * 2), tok = arena.alloc((int64_t)Tx * C * 4 * 4);
        const bool fp8 = E.fp8;
        const int64_t hx8 = fp8 ? arena.alloc((int64_t)Tx * D) : 0, sx = fp8 ? arena.alloc((int64_t)Tx * 4) : 0;
        const int64_t o8 = fp8 ? arena.alloc((int64_t)Tp * D) : 0, omx = fp8 ? arena.alloc((int64_t)Tp * D / 32) : 0;       // attention output, e4m3 + MX scales
        const int64_t f8 = fp8 ? arena.alloc((int64_t)Tx * 4 * D) : 0, fmx = fp8 ? arena.alloc((int64_t)Tx * 4 * D / 32) : 0;  // GELU(fc1) of the image stream
        const int64_t mx_slack = fp8 ? arena.alloc(2048) : 0;         // a 256-row scale piece may reach past the last plane (small grids, text rows)
        (void)mx_slack;

        op([=](const Ctx& c) {                                      // embeddings and conditioning
            // V^T columns past the joint sequence must be finite: P is exactly 0 there, 0 * garbage must be 0
            // ... and the q | k rows past it must be the same whatever the workspace held: the padded KEYS are masked, but the padded QUERIES share waves with real ones
            // (rows 4,416 .. 4,447 at SD3's 4,429 tokens), and k_flash_attn64_v2 re-references a WAVE when any of its scores passes the threshold -- exact up to the
            // bf16 rounding of P, so finite garbage there moved the real rows' last bits (and, in the fp8 engine, e4m3 roundings downstream: 3.7e-3 of the output;
            // round-4 review, weak #1; tools/diag_fp8_ws.py).  NaN garbage never did (a NaN compares false), which is why the NaN-poisoned workspace test missed it.
            if (Tp > Tx + Tc) {
                (void)hipMemset2DAsync(c.at<bf16>(vT) + Tx + Tc, (size_t)Tp * 2, 0, (size_t)(Tp - Tx - Tc) * 2, (size_t)c.B * D, c.stream);
                (void)hipMemset2DAsync(c.at<bf16>(qk) + (int64_t)(Tx + Tc) * 2 * D, (size_t)Tp * 2 * D * 2, 0, (size_t)(Tp - Tx - Tc) * 2 * D * 2, (size_t)c.B, c.stream);
            }
            const int64_t prow = (int64_t)c.B * Tx;
            launch_patch_embed(c.x, c.w<float>(w_pw), c.w<float>(w_pb), c.w<float>(w_pos), c.at<float>(x), C, gr, D, prow, s16, c.site(0), c.stream);
            launch_dit_time_freq(c.labels, c.at<bf16>(tf), c.B, c.stream);
            const int64_t np = (int64_t)c.B * Pd, nt = (int64_t)c.B * Tc * Jd;
            launch_f32_to_bf16(eng->pooled, c.at<bf16>(pl), np, c.stream);
            launch_f32_to_bf16(eng->text, c.at<bf16>(tx), nt, c.stream);
            launch_gemm(dense(c, c.at<bf16>(tf), 256, c.B, t1, D, ACT_SILU, c.at<bf16>(a1), OUT_BF16), c.stream);
            launch_gemm(dense(c, c.at<bf16>(a1), D, c.B, t2, D, ACT_NONE, c.at<float>(cf), OUT_F32), c.stream);
            launch_gemm(dense(c, c.at<bf16>(pl), Pd, c.B, x1, D, ACT_SILU, c.at<bf16>(a2), OUT_BF16), c.stream);
            GemmArgs g = dense(c, c.at<bf16>(a2), D, c.B, x2, D, ACT_NONE, c.at<float>(cf), OUT_F32);      // c = t_emb + pooled_emb
            g.resid_f32 = c.at<float>(cf); g.resid_f32_ld = D;
            launch_gemm(g, c.stream);
            launch_silu_bf16(c.at<float>(cf), c.at<bf16>(cs), (int64_t)c.B * D, c.stream);
            launch_gemm(dense(c, c.at<bf16>(cs), D, c.B, Lin{w_mod, b_mod}, nmod, ACT_NONE, c.at<float>(mod), OUT_F32), c.stream);      // every adaLN linear at once
            launch_gemm(dense(c, c.at<bf16>(tx), Jd, c.B * Tc, ce, D, ACT_NONE, c.at<float>(e), OUT_F32), c.stream);   // context_embedder
        });

        auto ln_mod = [=](int64_t src, int rows_per_seq, int shift_off, int scale_off, int64_t dst) {
            const bool src16 = s16 && src == x;                       // (the image stream in half; the text stream e is fp32)
            return [=](const Ctx& c) {
                const int64_t rows = (int64_t)c.B * rows_per_seq;
                launch_ln_modulate<RowsBf16>(c.at<float>(src), c.at<float>(mod) + shift_off, c.at<float>(mod) + scale_off, nmod, c.at<bf16>(dst), nullptr, D, rows, rows_per_seq, c.stream, src16);
            };
        };
        auto ln_mod8 = [=](int shift_off, int scale_off) {         // image stream -> fp8 rows + per-token scales
            return [=](const Ctx& c) {
                const int64_t rows = (int64_t)c.B * Tx;
                launch_ln_modulate<RowsFp8>(c.at<float>(x), c.at<float>(mod) + shift_off, c.at<float>(mod) + scale_off, nmod, c.at<uint8_t>(hx8), c.at<float>(sx), D, rows, Tx,
                                   c.stream, s16);
            };
        };
        // stream += gate * (. + bias), one sequence per batch index; site: the launch's slot of the stream guard (image stream only).  The image stream may be half
        // (g.c is the same stream: both sides of the update are half rows then)
        auto update = [=](GemmArgs g, const Ctx& c, int gate_off, int64_t stream_off, int site = -1) {
            return gated(g, c.at<float>(mod) + gate_off, nmod, 30, 1, c.at<float>(stream_off), D, s16 && stream_off == x, site >= 0 ? c.site(site) : nullptr);
        };

        // the text stream's launches: on Ctx::stream2 when the forward has one (natinf_set_mmdit_text_stream), joined with the image stream by events where the
        // two meet -- in front of the joint attention (text q | k | v written) and behind it (the text stream's output projection reads its rows of O)
        auto on_text = [](OpFn f) { return OpFn([f](const Ctx& c) { if (!c.stream2) { f(c); return; } Ctx t = c; t.stream = c.stream2; f(t); }); };
        auto ev_record = [](int i, bool text) { return OpFn([=](const Ctx& c) { if (c.stream2) (void)hipEventRecord(c.ev[i], text ? c.stream2 : c.stream); }); };
        auto ev_wait = [](int i, bool text) { return OpFn([=](const Ctx& c) { if (c.stream2) (void)hipStreamWaitEvent(text ? c.stream2 : c.stream, c.ev[i], 0); }); };
        op(ev_record(0, false)); op(ev_wait(0, true));           // fork: the modulation vectors and the embedded context are written

        int moff = 0;
        for (int i = 0; i < L; ++i) {
            const bool last = i == L - 1;
            const int mx = moff, me = moff + 6 * D;                  // x: shift, scale, gate (msa) | shift, scale, gate (mlp)
            linear_at(6 * D, D, w_mod + (int64_t)mx * D * 2, b_mod + (int64_t)mx * 4);
            linear_at((last ? 2 : 6) * D, D, w_mod + (int64_t)me * D * 2, b_mod + (int64_t)me * 4);
            moff += (last ? 8 : 12) * D;
            // q|k stacks and v per stream; parameter order: to_q, to_k, to_v, add_k_proj, add_v_proj, add_q_proj
            const int64_t w_qkx = wres((int64_t)2 * D * D * 2), b_qkx = wres((int64_t)2 * D * 4);
            const int64_t w_qke = wres((int64_t)2 * D * D * 2), b_qke = wres((int64_t)2 * D * 4);
            const int64_t w_qk8 = fp8 ? wres((int64_t)2 * D * D) : 0, s_qk8 = fp8 ? wres((int64_t)2 * D * 4) : 0;
            Lin vx{0, 0};
            Lin8 vx8{0, 0, 0};
            if (fp8) {
                int64_t pw = take((int64_t)D * D), pb = take(D);                             // to_q
                pack_fp8_at(pw, D, D, w_qk8, s_qk8); pack_f32_at(pb, D, b_qkx);
                pw = take((int64_t)D * D); pb = take(D);                                     // to_k
                pack_fp8_at(pw, D, D, w_qk8 + (int64_t)D * D, s_qk8 + (int64_t)D * 4); pack_f32_at(pb, D, b_qkx + (int64_t)D * 4);
                vx8 = linear8(D, D);                                                         // to_v
            } else {
                linear_at(D, D, w_qkx, b_qkx);                                               // to_q
                linear_at(D, D, w_qkx + (int64_t)D * D * 2, b_qkx + (int64_t)D * 4);         // to_k
                vx = linear(D, D);                                                           // to_v
            }
            linear_at(D, D, w_qke + (int64_t)D * D * 2, b_qke + (int64_t)D * 4);             // add_k_proj
            const Lin ve = linear(D, D);                                                     // add_v_proj
            linear_at(D, D, w_qke, b_qke);                                                   // add_q_proj
            Lin ox{0, 0}, oe{0, 0};
            Lin8 ox8{0, 0, 0}, oe8{0, 0, 0};
            if (fp8) { ox8 = linear8(D, D); if (!last) oe8 = linear8(D, D); }
            else { ox = linear(D, D); if (!last) oe = linear(D, D); }
            Lin f1{0, 0};
            Lin8 f18{0, 0, 0};
            if (fp8) f18 = linear8(4 * D, D); else f1 = linear(4 * D, D);
            Lin f2{0, 0};
            Lin8 f28{0, 0, 0};
            if (fp8) f28 = linear8(D, 4 * D); else f2 = linear(D, 4 * D);
            const Lin g1 = last ? Lin{0, 0} : linear(4 * D, D), g2 = last ? Lin{0, 0} : linear(D, 4 * D);
            const Lin qkx{w_qkx, b_qkx}, qke{w_qke, b_qke};

            op(fp8 ? OpFn(ln_mod8(mx, mx + D)) : OpFn(ln_mod(x, Tx, mx, mx + D, hx)));
            // text stream: adaLN-Zero (shift, scale, ...) or, in the last block, AdaLayerNormContinuous (scale, shift)
            op(on_text(last ? ln_mod(e, Tc, me + D, me, he) : ln_mod(e, Tc, me, me + D, he)));
            const Lin8 qkx8{w_qk8, s_qk8, b_qkx};
            const int64_t qk_bs = (int64_t)Tp * 2 * D;
            op([=](const Ctx& c) {                          // image stream: q | k into rows [0, Tx) of the joint buffer, V^T columns [0, Tx)
                if (fp8) {                                  // on e4m3 operands
                    GemmArgs g = seq_gemm(c, nullptr, D, (int64_t)Tx * D, Tx, qkx8, 2 * D, c.at<bf16>(qk), 2 * D, qk_bs, OUT_BF16);
                    a_fp8_rows(g, c.at<uint8_t>(hx8), c.at<float>(sx), Tx);
                    launch_gemm_fp8(g, c.stream);
                    launch_gemm_fp8(vt8(c, vx8, D, c.at<uint8_t>(hx8), c.at<float>(sx), Tx, c.at<bf16>(vT), Tp), c.stream);
                } else {
                    launch_gemm(seq_gemm(c, c.at<bf16>(hx), D, (int64_t)Tx * D, Tx, qkx, 2 * D, c.at<bf16>(qk), 2 * D, qk_bs, OUT_BF16), c.stream);
                    launch_gemm(vt(c, vx, D, c.at<bf16>(hx), Tx, c.at<bf16>(vT), Tp), c.stream);
                }
            });
            op(on_text([=](const Ctx& c) {                  // text stream: rows / columns [Tx, Tx + Tc)
                launch_gemm(seq_gemm(c, c.at<bf16>(he), D, (int64_t)Tc * D, Tc, qke, 2 * D, c.at<bf16>(qk) + (int64_t)Tx * 2 * D, 2 * D, qk_bs, OUT_BF16), c.stream);
                launch_gemm(vt(c, ve, D, c.at<bf16>(he), Tc, c.at<bf16>(vT), Tp, Tx), c.stream);
            }));
            op(ev_record(1 + 2 * i, true)); op(ev_wait(1 + 2 * i, false));          // the joint attention needs both
            op([=](const Ctx& c) {
                if (fp8) {
                    launch_flash(c.at<bf16>(qk), c.at<bf16>(qk) + D, 2 * D, qk_bs, c.at<bf16>(vT), nullptr, D, (int64_t)Tp * D, c.B, H, Tp,
                                 Tx + Tc, 0.125f, c.stream, c.at<uint8_t>(o8), c.at<uint8_t>(omx));
                } else {
                    launch_flash(c.at<bf16>(qk), c.at<bf16>(qk) + D, 2 * D, qk_bs, c.at<bf16>(vT), c.at<bf16>(o), D, (int64_t)Tp * D, c.B, H, Tp,
                                 Tx + Tc, 0.125f, c.stream);
                }
            });
            op(ev_record(2 + 2 * i, false));
            // stream += gate * (O W^T + b) for rows [row0, row0 + T) of the joint attention output: bf16 rows, or (fp8) e4m3 rows + MX scales in K-tile-major planes of Tp rows
            auto proj = [=](const Ctx& c, const Lin& w, const Lin8& w8, int row0, int T, int64_t stream_off, int gate_off, int site = -1) {
                if (fp8) {
                    GemmArgs g = seq_gemm(c, nullptr, D, (int64_t)Tp * D, T, w8, D, c.at<float>(stream_off), D, (int64_t)T * D, OUT_F32);
                    a_fp8_mx(g, c.at<uint8_t>(o8) + (int64_t)row0 * D, c.at<uint8_t>(omx) + (int64_t)row0 * 4, Tp, (int64_t)Tp * (D / 32));
                    launch_gemm_fp8(update(g, c, gate_off, stream_off, site), c.stream);
                } else {
                    launch_gemm(update(seq_gemm(c, c.at<bf16>(o) + (int64_t)row0 * D, D, (int64_t)Tp * D, T, w, D, c.at<float>(stream_off), D, (int64_t)T * D, OUT_F32), c, gate_off, stream_off, site),
                                c.stream);
                }
            };
            op([=](const Ctx& c) { proj(c, ox, ox8, 0, Tx, x, mx + 2 * D, 1 + 2 * i); });                  // image stream's output projection
            if (!last) {
                op(ev_wait(2 + 2 * i, true));
                op(on_text([=](const Ctx& c) { proj(c, oe, oe8, Tx, Tc, e, me + 2 * D); }));             // text stream's output projection
            }
            op(fp8 ? OpFn(ln_mod8(mx + 3 * D, mx + 4 * D)) : OpFn(ln_mod(x, Tx, mx + 3 * D, mx + 4 * D, hx)));
            op([=](const Ctx& c) {
                if (fp8) {
                    const int64_t mx_bs = (int64_t)Tx * (4 * D / 32);
                    GemmArgs g = seq_gemm(c, nullptr, D, (int64_t)Tx * D, Tx, f18, 4 * D, c.at<uint8_t>(f8), 4 * D, (int64_t)Tx * 4 * D, OUT_FP8_MX);      // e4m3 + a scale per 32 columns: fc2's operand
                    a_fp8_rows(g, c.at<uint8_t>(hx8), c.at<float>(sx), Tx);
                    g.act = ACT_GELU_TANH; g.c_mx = c.at<uint8_t>(fmx); g.c_mx_ld = Tx; g.c_mx_bs = mx_bs;
                    launch_gemm_fp8(g, c.stream);
                    g = seq_gemm(c, nullptr, 4 * D, (int64_t)Tx * 4 * D, Tx, f28, D, c.at<float>(x), D, (int64_t)Tx * D, OUT_F32);                          // x += gate_mlp * (f8 W2^T + b)
                    a_fp8_mx(g, c.at<uint8_t>(f8), c.at<uint8_t>(fmx), Tx, mx_bs);
                    launch_gemm_fp8(update(g, c, mx + 5 * D, x, 2 + 2 * i), c.stream);
                    return;
                }
                GemmArgs g = seq_gemm(c, c.at<bf16>(hx), D, (int64_t)Tx * D, Tx, f1, 4 * D, c.at<bf16>(fx), 4 * D, (int64_t)Tx * 4 * D, OUT_BF16);
                g.act = ACT_GELU_TANH;
                launch_gemm(g, c.stream);
                launch_gemm(update(seq_gemm(c, c.at<bf16>(fx), 4 * D, (int64_t)Tx * 4 * D, Tx, f2, D, c.at<float>(x), D, (int64_t)Tx * D, OUT_F32), c, mx + 5 * D, x, 2 + 2 * i), c.stream);
            });
            if (!last) {
                op(on_text(ln_mod(e, Tc, me + 3 * D, me + 4 * D, he)));
                op(on_text([=](const Ctx& c) {
                    // the text stream's fc1 has no per-sequence term (bias + GELU) and both its operands are contiguous over the sequences: ONE GEMM over B * Tc rows
                    // (natinf_set_mmdit_text_flat) instead of B batched ones of Tc = 333 rows each -- 11 row tiles of 256 for 8 sequences instead of 16
                    GemmArgs g = g_mmdit_text_flat ? dense(c, c.at<bf16>(he), D, c.B * Tc, g1, 4 * D, ACT_GELU_TANH, c.at<bf16>(fe), OUT_BF16)
                                                   : seq_gemm(c, c.at<bf16>(he), D, (int64_t)Tc * D, Tc, g1, 4 * D, c.at<bf16>(fe), 4 * D, (int64_t)Tc * 4 * D, OUT_BF16);
                    g.act = ACT_GELU_TANH;
                    launch_gemm(g, c.stream);
                    launch_gemm(update(seq_gemm(c, c.at<bf16>(fe), 4 * D, (int64_t)Tc * 4 * D, Tc, g2, D, c.at<float>(e), D, (int64_t)Tc * D, OUT_F32), c, me + 5 * D, e), c.stream);
                }));
            }
        }
        op(ev_record(2 * L + 1, true)); op(ev_wait(2 * L + 1, false));               // join: nothing of this forward is left on the text stream's queue
        // ---- norm_out (scale, shift), proj_out, unpatchify
        const int mo = moff;
        linear_at(2 * D, D, w_mod + (int64_t)mo * D * 2, b_mod + (int64_t)mo * 4);
        const Lin po = linear(4 * C, D);
        op(ln_mod(x, Tx, mo + D, mo, hx));
        op([=](const Ctx& c) {
            launch_gemm(dense(c, c.at<bf16>(hx), D, c.B * Tx, po, 4 * C, ACT_NONE, c.at<float>(tok), OUT_F32), c.stream);
            launch_unpatchify(c.at<float>(tok), c.out, C, gr, c.B, c.stream);
        });
        finish();
    }
};

}  // namespace

extern "C" {

int natinf_mmdit_create(natinf_mmdit_t* out, int layers, int heads, int joint_dim, int pooled_dim, int in_ch, int grid, int ctx_tokens, int flags) {
    if (!out || (flags & ~(NATINF_MMDIT_FP8 | NATINF_MMDIT_STREAM_GUARD)) || ((flags & NATINF_MMDIT_FP8) && heads % 2) || layers <= 0 || heads <= 0 || heads * 64 > 1536 || joint_dim <= 0 || joint_dim % 8 || pooled_dim <= 0 || pooled_dim % 8 ||
        in_ch <= 0 || in_ch > 16 || (in_ch * 4) % 8 || grid <= 0 || (grid * grid) % 8 || ctx_tokens <= 0)
        return NATINF_EINVAL;
    natinf_mmdit* e = new natinf_mmdit();
    e->L = layers; e->H = heads; e->D = heads * 64; e->Jd = joint_dim; e->Pd = pooled_dim; e->C = in_ch; e->g = grid;
    e->Tx = grid * grid; e->Tc = ctx_tokens; e->Tp = (int)align_up(e->Tx + e->Tc, 128);
    e->fp8 = (flags & NATINF_MMDIT_FP8) != 0;
    e->stream16 = g_mmdit_stream16 != 0;
    e->guard_sites = (flags & NATINF_MMDIT_STREAM_GUARD) ? 1 + 2 * layers : 0;      // the image stream: patch embedding, then per block the attention-projection and the MLP update (the text stream is fp32: unguarded)
    MMDitBuilder b(*e);
    b.build();
    *out = e;
    return NATINF_OK;
}
int natinf_mmdit_destroy(natinf_mmdit_t h) { if (!h) return NATINF_EINVAL; delete h; return NATINF_OK; }
int64_t natinf_mmdit_param_count(natinf_mmdit_t h) { return h ? h->n_params : NATINF_EINVAL; }
int64_t natinf_mmdit_packed_bytes(natinf_mmdit_t h) { return h ? h->packed_bytes : NATINF_EINVAL; }
int64_t natinf_mmdit_workspace_bytes(natinf_mmdit_t h, int max_batch) { return h && max_batch > 0 ? h->workspace_bytes(max_batch) : NATINF_EINVAL; }
int natinf_mmdit_stream_sites(natinf_mmdit_t h) { return h && h->guard_sites ? h->guard_sites : NATINF_EINVAL; }
int natinf_mmdit_stream_status_reset(natinf_mmdit_t h, void* workspace, natinf_stream_t stream) { return h ? h->status_reset(workspace, (hipStream_t)stream) : NATINF_EINVAL; }
int natinf_mmdit_stream_status(natinf_mmdit_t h, const void* workspace, uint32_t* out_dev, natinf_stream_t stream) { return h ? h->status_read(workspace, out_dev, (hipStream_t)stream) : NATINF_EINVAL; }

int natinf_mmdit_load(natinf_mmdit_t h, const float* params_f32, int64_t n_params, void* packed, int64_t packed_bytes, natinf_stream_t stream) {
    return h ? h->load(params_f32, n_params, packed, packed_bytes, (hipStream_t)stream) : NATINF_EINVAL;
}

int natinf_mmdit_forward(natinf_mmdit_t h, const float* latents, const float* timestep, const float* text, const float* pooled, float* out,
                         int B, void* workspace, int64_t workspace_bytes, natinf_stream_t stream) {
    if (!h || !text || !pooled) return NATINF_EINVAL;
    h->text = text; h->pooled = pooled;
    const bool two = g_mmdit_text_stream && h->ensure_aux();
    return h->run(latents, timestep, out, B, workspace, workspace_bytes, (hipStream_t)stream, two ? h->aux : nullptr, two ? h->ev.data() : nullptr);
}

int natinf_attention_hd64_bf16(const void* q, const void* k, int ld_qk, int64_t qk_bs, const void* vT, void* o, int ld_o, int64_t o_bs,
                               int B, int H, int Tp, int T, float scale, natinf_stream_t stream) {
    if (!q || !k || !vT || !o || B <= 0 || H <= 0 || Tp <= 0 || Tp % 128 || T <= 0 || T > Tp || Tp - T >= 128 || ld_qk % 8 || ld_o % 4) return NATINF_EINVAL;      // only the LAST key tile is masked
    if (!configure_gemm_kernels()) return NATINF_ENODEV;
    launch_flash((const bf16*)q, (const bf16*)k, ld_qk, qk_bs, (const bf16*)vT, (bf16*)o, ld_o, o_bs, B, H, Tp, T, scale, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

// test hook: the fp8 output epilogue of the current flash mode's kernel on its own (what the fp8 engine hands to its output projection)
int natinf_debug_attention_hd64_fp8out(const void* q, const void* k, int ld_qk, int64_t qk_bs, const void* vT, void* o8, void* omx, int B, int H, int Tp,
                                       int T, float scale, natinf_stream_t stream) {
    if (!q || !k || !vT || !o8 || !omx || B <= 0 || H <= 0 || H % 2 || Tp <= 0 || Tp % 128 || T <= 0 || T > Tp || Tp - T >= 128 || ld_qk % 8) return NATINF_EINVAL;      // (H: a scale plane pairs heads)
    if (!configure_gemm_kernels()) return NATINF_ENODEV;
    launch_flash((const bf16*)q, (const bf16*)k, ld_qk, qk_bs, (const bf16*)vT, nullptr, 64 * H, (int64_t)Tp * 64 * H, B, H, Tp, T, scale, (hipStream_t)stream,
                 (uint8_t*)o8, (uint8_t*)omx);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_set_flash_mode(int mode) {
    if (mode < 0 || mode > 3) return NATINF_EINVAL;
    if (mode == 1 || mode == 2) return NATINF_ESTATE;       // the intermediate forms (vector-pipe row sums; 128-key tiles): retired
    g_flash_mode = mode;
    return NATINF_OK;
}
int natinf_set_mmdit_text_stream(int on) { g_mmdit_text_stream = on != 0; return NATINF_OK; }
int natinf_set_mmdit_text_flat(int on) { g_mmdit_text_flat = on != 0; return NATINF_OK; }
int natinf_set_mmdit_stream16(int on) { g_mmdit_stream16 = on < 0 ? MMDIT_STREAM16_DEFAULT : (on != 0); return NATINF_OK; }
int natinf_attention_profile(int enable) { g_flash_prof.on = enable != 0; return NATINF_OK; }
int natinf_attention_profile_read(double* ms_total, int64_t* launches) {
    if (!ms_total || !launches) return NATINF_EINVAL;
    *ms_total = 0.0; *launches = 0;
    for (auto& e : g_flash_prof.ev) {
        float ms = 0.f;
        if (hipEventSynchronize(e.second) != hipSuccess || hipEventElapsedTime(&ms, e.first, e.second) != hipSuccess) { (void)hipGetLastError(); return NATINF_ELAUNCH; }
        *ms_total += ms; *launches += 1;
        g_flash_prof.pool.push_back(e);
    }
    g_flash_prof.ev.clear();
    return NATINF_OK;
}

}  // extern "C"
