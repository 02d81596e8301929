// ncsnpp.hip -- the one translation unit of the engines.  Its own code is the host side of the NCSN++ denoiser engine: the static execution
// plan (Builder), weight packing, forward; the C ABI of include/natinf_ncsnpp.h with the natinf_debug_* / natinf_set_* entries.  The GEMM
// launch layer every engine calls is gemm_launch.h, the engine base and the plan builder's shared recipes engine_core.h, the kernels
// ncsnpp_kernels.h and the headers below; the other four engines are included at the end of this file (the two transformer engines bring their
// own shared pieces: the row and glue kernels of transformer_rows.h, the plan base and GEMM recipes of transformer_plan.h).
//
// Design (MI355X-first, not a translation of the reference's nn.Module tree):
//   * the network is compiled once into a flat op list (~330 launches) over ONE caller-supplied
//     workspace; every tensor offset is "bytes per image", so a plan built once serves any batch;
//   * activations are NHWC bf16; U-Net skip tensors are written by their producer straight into the
//     channel slice of the concat buffer their consumer will read (no torch.cat copies), and an up-path
//     block writes its output into the first channel slice of the next block's concat buffer;
//   * a res-block is 6 launches: GN-stats, GN-apply(+SiLU, +up/down of both branches), conv3x3 GEMM
//     (+bias +time-embedding row), GN-stats, GN-apply, conv3x3 GEMM whose K range is extended by the
//     1x1 shortcut conv (one GEMM computes Conv_1(h) + Conv_2(x)) with the residual add and the
//     1/sqrt(2) rescale in its epilogue;
//   * the 44 per-block time-embedding projections (Dense_0) are one GEMM at the top of the forward.
//
// Reference: deps/score_sde_pytorch/models/ncsnpp.py:232-381, layerspp.py:75-91,242-274,
// layers.py:515-555, up_or_down_sampling.py:59-69.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "natinf_ncsnpp.h"
#include "gemm_launch.h"
#include "engine_core.h"
#include "head_conv.h"
#include "attn256.h"
#include "attn_qkv.h"
#include "attn_blk256.h"

namespace {

constexpr int NF = 128, IMG = 32, TEMB = 512, NLEVEL = 4;      // res-blocks per level: 4 (cifar10_ddpmpp_continuous) or 2 (the `ddpm` network), Builder::NUM_RES
constexpr int CH_MULT[NLEVEL] = {1, 2, 2, 2};
constexpr float GN_EPS = 1e-6f;
constexpr float INV_SQRT2 = 0.70710678118654752440f;
inline bool attn_at(int res) { return res == 16; }

enum Kind { K_LIN, K_CONV, K_RES, K_ATTN, K_GN, K_DOWN, K_UP };      // K_DOWN / K_UP: the plain resampling convolutions of the `ddpm` network
const char* kind_name(int k) { static const char* n[] = {"lin", "conv", "res", "attn", "gn", "down", "up"}; return n[k]; }

struct Mod { int idx, kind, cin, cout, up, down, res; int64_t poff; };

enum { CLS_GEMM = 0, CLS_OTHER = 1, CLS_CONV_GN = 2, CLS_CONV_GN8 = 3, N_CLS = 4 };      // CLS_CONV_GN: launches of the fused GroupNorm + SiLU + 3x3 conv kernel at 32x32 / 16x16; CLS_CONV_GN8: its 8x8 instantiation

int g_fuse_head = 1;               // natinf_set_fuse_head (read when a plan is BUILT): GroupNorm + SiLU + the 128 -> 3 output convolution as ONE launch (head_conv.h)
constexpr int ATTN_BLK_DEFAULT = 2;
int g_attn_blk = ATTN_BLK_DEFAULT;  // natinf_set_attn_block (read when a plan is BUILT): the whole 16x16 attention block as ONE launch -- 1: k_qkv256 + k_attn256<true, 8> in one kernel (attn_blk256.h: q stays in
                                   // registers, k / V^T through L2); 2 (default since round 6): k_attn_blk256_v2 -- q k^T and P V against h itself, h resident in LDS (forward -3.3 % at B = 512); 0: two launches
int g_attn_qkv = 1;                // natinf_set_attn_qkv (read when a plan is BUILT): GroupNorm-apply + the q | k | v projections of the 16x16 attention as ONE launch (attn_qkv.h)
int g_attn_w8 = 1;                 // natinf_set_attn_waves8: k_attn256<true> as one 8-wave block per sample (1) or two 4-wave blocks (0)
int g_attn_proj = 1;               // natinf_set_attn_proj (read when a plan is BUILT): the 16x16 attention's output projection + skip + GroupNorm partials inside k_attn256
int g_fuse_gn8 = 1;                // natinf_set_fuse_gn8 (read when a plan is BUILT): the 8x8 level on the fused kernel too (two images per 128-pixel tile)
int g_fuse_fin = 3;                // natinf_set_fuse_fin (read when a plan is BUILT): at 8x8 / 4x4 the fused convolution's epilogue writes the GroupNorm table of its
                                   // output's consumer itself (whole samples x all channels per tile) instead of a k_gn_finalize launch behind it
int g_fuse_gn4 = 1;                // natinf_set_fuse_gn4 (read when a plan is BUILT): the 4x4 level on the fused kernel too (four images per 64-pixel tile) instead of
                                   // k_gn_apply + split-K GEMM + k_splitk_reduce + k_gn_stats
int g_fuse_gn = 1;                 // natinf_set_fuse_gn (read when a plan is BUILT): GroupNorm-apply + SiLU inside the consuming 3x3 conv
constexpr int UP_FOLD_DEFAULT = 1;
int g_fuse_up_fold = UP_FOLD_DEFAULT;   // natinf_set_fuse_up_fold (read when a plan is BUILT): Conv_0 of the 16 -> 32 up-sampling block as four 2x2 phase convolutions over its 16x16 input
                                   // (k_fold_up_conv + k_gn_apply at 16x16 + k_conv_gn_upfold: 4/9 of the multiply-accumulates) instead of a nine-tap launch with the up-sampling in its fetch
int g_fuse_up = 1;                 // natinf_set_fuse_up (read when a plan is BUILT): up blocks at 16x16 / 32x32 fetch their input up-sampled inside k_conv_gn2

}  // namespace

struct natinf_ncsnpp : EngineCore {
    int flags = 0;
    std::vector<Mod> mods;
    std::vector<int> op_cls;             // CLS_* per op (profiling)
    // profiling: one HIP event pair per op while enabled
    bool prof = false;
    struct Rec { hipEvent_t a, b; int cls; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    std::map<int, TRef> taps;            // module idx -> output tensor
    uint64_t plan_sig = 0;               // the natinf_set_* switches a plan reads when it is BUILT (they decide the pack offsets): natinf_ncsnpp_share compares them
    int last_B = 0; unsigned char* last_ws = nullptr;
    std::vector<unsigned char> fin_done; // see Ctx::fin_done
};

namespace {

// LDS sizes of the kernels only this engine launches (configure_gemm_kernels, gemm_launch.h)
bool configure_ncsnpp_kernels() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_head_conv), hipFuncAttributeMaxDynamicSharedMemorySize, HeadConvCfg::LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&k_qkv256), hipFuncAttributeMaxDynamicSharedMemorySize, QKV_LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn256<false>), hipFuncAttributeMaxDynamicSharedMemorySize, A256_LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn256<true>), hipFuncAttributeMaxDynamicSharedMemorySize, A256_LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn256<true, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, A256_LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_blk256), hipFuncAttributeMaxDynamicSharedMemorySize, ABLK_LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_blk256_v2), hipFuncAttributeMaxDynamicSharedMemorySize, ABLK2_LDS_BYTES) == hipSuccess;
}

// ------------------------------------------------------------------------------------------------
// the 16x16 attention block (256 tokens, 256 channels): its weight packs and its launches -- ONE copy, called by the plan builder (Builder::emit_attn)
// and by natinf_debug_attn_block
// ------------------------------------------------------------------------------------------------
struct AttnBlk256 {
    int plan = 0;                    // 2: k_attn_blk256_v2; 1: k_attn_blk256; 0: k_qkv256 (launch_attn_qkv256, or the GEMMs that write the same tensors) + k_attn256<true>
    int B = 0;
    const bf16* x = nullptr; int x_ld = 0;                             // raw block input (normalised for the projections; the residual of the output)
    const float* sc = nullptr; const float* sh = nullptr;              // GroupNorm (scale | shift) tables [B][256]
    const bf16* wqkvf = nullptr; const float* bqk = nullptr; const float* bv = nullptr; bf16* qk = nullptr; bf16* vT = nullptr;      // plans 0 / 1 (pack_attn_qkv_w; [q | k] and V^T scratch)
    const bf16* w3f = nullptr; const float* b3 = nullptr;              // plans 0 / 1 (pack_attn_w3)
    const bf16* wqf2 = nullptr; const float* cq2 = nullptr; const bf16* wvof2 = nullptr; const float* bo2 = nullptr;                  // plan 2 (pack_attn_fold)
    bf16* out = nullptr; int o_ld = 0; float out_scale = 1.0f;
    float2* gn_part = nullptr; int gn_quads = 0;
};
void pack_attn_qkv_w(const float* w0, const float* w1, const float* w2, bf16* wqkvf, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_qkv_w, dim3(3 * 256), dim3(256), 0, s, w0, w1, w2, wqkvf);
}
void pack_attn_w3(const float* w3, bf16* w3f, hipStream_t s) { hipLaunchKernelGGL(k_pack_attn_w3, dim3(256), dim3(256), 0, s, w3, w3f); }
// the folded matrices of k_attn_blk256_v2: Wqk = Wq Wk^T, cq = bq Wk^T, Wvo = Wv W3, bo = bv W3 + b3 in fp32 (fq / fv: [256][256] temporaries), packed like the q tiles / W3 of the four-projection plans
void pack_attn_fold(const float* w0, const float* w1, const float* w2, const float* w3, const float* b0, const float* b2, const float* b3,
                    float* fq, float* cq, float* fv, float* bo, bf16* wqf2, bf16* wvof2, hipStream_t s) {
    hipLaunchKernelGGL(k_attn_fold_w, dim3(257), dim3(256), 0, s, w0, w1, w2, w3, b0, b2, b3, fq, cq, fv, bo);
    hipLaunchKernelGGL(k_pack_qkv_w, dim3(256), dim3(256), 0, s, (const float*)fq, (const float*)fq, (const float*)fq, wqf2, 1);
    hipLaunchKernelGGL(k_pack_attn_w3, dim3(256), dim3(256), 0, s, (const float*)fv, wvof2);
}
void launch_attn_qkv256(const AttnBlk256& a, hipStream_t s) {          // plan 0's first launch: x -> [q | k], V^T
    hipLaunchKernelGGL(k_qkv256, dim3((unsigned)a.B), dim3(512), QKV_LDS_BYTES, s, a.x, a.x_ld, a.sc, a.sh, a.wqkvf, a.bqk, a.bv, a.qk, a.vT);
}
// returns the rows one GroupNorm partial row of the launch covers (Ctx::part_bm): a sample, or its half (k_attn256<true> as two 4-wave blocks)
int launch_attn_blk256(const AttnBlk256& a, hipStream_t s) {
    constexpr int C = 256;
    if (a.plan == 2) {
        hipLaunchKernelGGL(k_attn_blk256_v2, dim3((unsigned)a.B), dim3(512), ABLK2_LDS_BYTES, s, a.x, a.x_ld, a.sc, a.sh,
                           a.wqf2, a.cq2, 1.0f / sqrtf((float)C), a.wvof2, a.bo2, a.out, a.o_ld, a.out_scale, a.gn_part, a.gn_quads);
        return 256;
    }
    if (a.plan == 1) {
        hipLaunchKernelGGL(k_attn_blk256, dim3((unsigned)a.B), dim3(512), ABLK_LDS_BYTES, s, a.x, a.x_ld, a.sc, a.sh,
                           a.wqkvf, a.bqk, a.bv, a.qk, a.vT, 1.0f / sqrtf((float)C), a.w3f, a.b3, a.out, a.o_ld, a.out_scale, a.gn_part, a.gn_quads);
        return 256;
    }
    if (g_attn_w8) {
        hipLaunchKernelGGL((k_attn256<true, 8>), dim3((unsigned)a.B), dim3(512), A256_LDS_BYTES, s, (const bf16*)a.qk, 2 * C, C, (const bf16*)a.vT, a.out, a.o_ld,
                           1.0f / sqrtf((float)C), a.w3f, a.b3, a.x, a.x_ld, a.out_scale, a.gn_part, a.gn_quads);
        return 256;
    }
    hipLaunchKernelGGL(k_attn256<true>, dim3((unsigned)(2 * a.B)), dim3(256), A256_LDS_BYTES, s, (const bf16*)a.qk, 2 * C, C, (const bf16*)a.vT, a.out, a.o_ld,
                       1.0f / sqrtf((float)C), a.w3f, a.b3, a.x, a.x_ld, a.out_scale, a.gn_part, a.gn_quads);
    return 128;
}

// ------------------------------------------------------------------------------------------------
// plan builder
// ------------------------------------------------------------------------------------------------
struct Builder : PlanBuilder {        // (wtop: the packed-weight bump pointer in bytes; poff: the running parameter offset in floats)
    natinf_ncsnpp& E;
    // time-embedding projection bank
    int dense_total = 0; int64_t dense_w = 0, dense_b = 0, dense_out = 0;

    // NATINF_NCSNPP_DDPM: the `ddpm` network (ddpm.py:39-181; configs/vp/ddpm/cifar10_continuous.py) -- two ResnetBlockDDPM per level (no
    // 1/sqrt(2) rescale, NIN shortcut), AttnBlock without rescale, Downsample / Upsample as plain 3x3 convolutions -- on the same kernels
    const bool ddpm;
    const int NUM_RES;
    const float res_scale;               // 1/sqrt(2) (skip_rescale of the ++ blocks) or 1
    explicit Builder(natinf_ncsnpp& e) : PlanBuilder(e), E(e), ddpm((e.flags & NATINF_NCSNPP_DDPM) != 0), NUM_RES(ddpm ? 2 : 4), res_scale(ddpm ? 1.0f : INV_SQRT2) {
        arena.keep = (e.flags & NATINF_NCSNPP_KEEP_ACTIVATIONS) != 0;
    }

    void op(int cls, OpFn f) { E.ops.push_back(std::move(f)); E.op_cls.push_back(cls); }

    // ---- weight packing recipes -------------------------------------------------------------
    void pack_conv(int64_t src, int64_t dst, int N, int Cin, int taps, int dst_ld, int koff, int tapstride, float wmul = 1.0f) {
        const int chunked = taps == 9 && Cin % BK == 0;      // every 3x3 conv except the 3-channel stem
        E.packs.push_back([=](const PackCtx& p) {
            const int64_t n = (int64_t)N * Cin * taps;
            hipLaunchKernelGGL(k_pack_conv, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream, p.params + src,
                               reinterpret_cast<bf16*>(p.packed + dst), N, Cin, taps, dst_ld, koff, tapstride, chunked, wmul);
        });
    }
    void pack_frag(int64_t src_packed, int64_t dst, int N, int ld, int cin, int c1) {      // packed -> packed (conv_gn2.h)
        E.packs.push_back([=](const PackCtx& p) {
            const int64_t n = (int64_t)(N / 16) * (9 * (cin / 32) + c1 / 32) * 64;
            hipLaunchKernelGGL(k_pack_frag, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream, reinterpret_cast<const bf16*>(p.packed + src_packed),
                               reinterpret_cast<bf16*>(p.packed + dst), N, ld, cin, c1);
        });
    }
    void pack_fold_up(int64_t src, int64_t dst, int N, int Cin, float wmul) {      // [N][Cin][3][3] fp32 -> the phase-major folded 2x2 kernels [4 N][4 Cin] bf16 (k_fold_up_conv)
        E.packs.push_back([=](const PackCtx& p) {
            ncsn_upf::fold(p.params + src, p.packed + dst, nullptr, N, Cin, wmul, (void*)p.stream);
        });
    }
    void pack_transpose(int64_t src, int64_t dst, int K, int N, int dst_ld) {
        E.packs.push_back([=](const PackCtx& p) {
            hipLaunchKernelGGL(k_pack_transpose, dim3(grid1d((int64_t)K * N, 256, 1 << 30)), dim3(256), 0, p.stream,
                               p.params + src, reinterpret_cast<bf16*>(p.packed + dst), K, N, dst_ld);
        });
    }
    void pack_zero(int64_t dst, int64_t n) {
        E.packs.push_back([=](const PackCtx& p) {
            hipLaunchKernelGGL(k_fill_bf16_zero, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream,
                               reinterpret_cast<bf16*>(p.packed + dst), n);
        });
    }
    // (fp32 vectors: PlanBuilder::pack_f32 / pack_f32_at; the longest one packed here is TEMB = 512 floats = two blocks)

    // ---- op emitters ------------------------------------------------------------------------
    struct GN { int64_t gamma, beta; };
    GN take_gn(int C) { GN g; g.gamma = pack_f32(take(C), C); g.beta = pack_f32(take(C), C); return g; }

    // GroupNorm statistics of x -> (scale, shift) per (image, channel); returns their arena offsets
    // (sc, sh: in / out -- where the producer's epilogue writes the table itself (Part::fin) they are REPLACED by its table)
    void emit_gn_stats(const TRef& x, GN gn, int64_t& sc, int64_t& sh, float out_mul = 1.0f) {
        if (emit_gn_from_parts(x, gn, sc, sh, out_mul)) return;
        const int HW = x.res * x.res;
        op(CLS_OTHER, [=](const Ctx& c) {
            hipLaunchKernelGGL(k_gn_stats, dim3(c.B), dim3(256), 0, c.stream, c.act(x), x.ld, x.C, HW,
                               c.w<float>(gn.gamma), c.w<float>(gn.beta), c.at<float>(sc), c.at<float>(sh), GN_EPS, out_mul);
        });
    }
    void emit_gn_apply(const TRef& x, int64_t sc, int64_t sh, const TRef& y, const TRef* xr, int act, int mode) {
        const int logW = ilog2(x.res), logHW = 2 * logW;
        const int rd = mode == RS_UP ? 2 * x.res : (mode == RS_DOWN ? x.res / 2 : x.res);
        const int rows_per_img = rd + 2 * y.pad;
        const TRef xrr = xr ? *xr : TRef();
        op(CLS_OTHER, [=](const Ctx& c) {
            hipLaunchKernelGGL(k_gn_apply, dim3((unsigned)((rows_per_img + GN_ROWS - 1) / GN_ROWS), (unsigned)c.B), dim3(256), 0, c.stream, c.act(x), x.ld, x.C,
                               logW, logHW, c.at<float>(sc), c.at<float>(sh), c.act(y),
                               xrr.off >= 0 ? c.act(xrr) : (bf16*)nullptr, act, mode, y.pad);
        });
    }
    TRef new_act(int res, int C, int pad = 0) {
        TRef t; t.off = arena.alloc((int64_t)(res + 2 * pad) * (res + 2 * pad) * C * 2); t.C = C; t.ld = C; t.res = res; t.pad = pad;
        return t;
    }

    void emit_res(const Mod& m, const TRef& x, const TRef& out) {
        const int cin = m.cin, cout = m.cout;
        const int ro = m.up ? m.res * 2 : (m.down ? m.res / 2 : m.res);
        const bool shortcut = cin != cout || m.up || m.down;
        // parameters in registration order (layerspp.py:204-228)
        const GN gn0 = take_gn(cin);
        const int64_t p_c0w = take((int64_t)cout * cin * 9), p_c0b = take(cout);
        const int64_t p_dw = take((int64_t)cout * TEMB), p_db = take(cout);
        const GN gn1 = take_gn(cout);
        const int64_t p_c1w = take((int64_t)cout * cout * 9), p_c1b = take(cout);
        const int64_t p_c2w = shortcut ? take((int64_t)cout * cin) : -1, p_c2b = shortcut ? take(cout) : -1;

        const int K0a = 9 * cin, K1tot = 9 * cout + (shortcut ? cin : 0);
        // GroupNorm-apply + SiLU inside the consuming convolution (conv_gn2.h) where an instantiation exists: output resolution
        // 32x32 or 16x16.  Conv_0 of a resampling block reads a resampled tensor and keeps the k_gn_apply pass (which also
        // produces the resampled shortcut input), Conv_1 is fused there too; the 8x8 / 4x4 levels are unfused.  Folded form: the
        // GroupNorm scale / shift carry -log2(e), the 3x3 weights -ln 2 (GemmArgs::gn_folded).
        const bool fusable_res = g_fuse_gn && (ro == 32 || ro == 16 || (ro == 8 && g_fuse_gn8 && cout % 256 == 0) || (ro == 4 && g_fuse_gn4 && cout % 256 == 0));
        const bool fuse1 = fusable_res && cout % BK == 0;                               // Conv_1
        const bool fuse_up = fuse1 && ro > 8 && g_fuse_up && m.up && cin % BK == 0 && cout % 128 == 0;   // up block: the 2x up-sampling of both branches happens in the fetches
        // ... or (natinf_set_fuse_up_fold, the 16 -> 32 block) not at all: Conv_0 runs as four 2x2 phase convolutions over the ACTIVATED 16x16 tensor -- a k_gn_apply pass at the low
        // resolution, then the up-fold launch (gemm_launch.h, up_fold.h) with the folded weights; Conv_1 and its shortcut segment keep the up-sampling fetch (a1_up)
        const bool fold_up = fuse_up && g_fuse_up_fold && !ddpm && ro == 2 * UPFOLD_W && cout == UPFOLD_BN;
        const bool fuse = (fusable_res && !m.up && !m.down && cin % BK == 0) || (fuse_up && !fold_up);            // Conv_0
        const float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
        const float gn_mul = fuse ? -LOG2E : 1.0f, w_mul = fuse ? -LN2 : 1.0f, gn_mul1 = fuse1 ? -LOG2E : 1.0f, w_mul1 = fuse1 ? -LN2 : 1.0f;
        const int64_t w0 = wres((int64_t)cout * (fold_up ? 16 * cin : K0a) * 2), w1 = wres((int64_t)cout * K1tot * 2);
        if (fold_up) pack_fold_up(p_c0w, w0, cout, cin, w_mul);
        else pack_conv(p_c0w, w0, cout, cin, 9, K0a, 0, cin, w_mul);
        pack_conv(p_c1w, w1, cout, cout, 9, K1tot, 0, cout, w_mul1);
        if (shortcut && !ddpm) pack_conv(p_c2w, w1, cout, cin, 1, K1tot, 9 * cout, cin);
        if (shortcut && ddpm) pack_transpose(p_c2w, w1 + (int64_t)9 * cout * 2, cin, cout, K1tot);      // NIN_0.W is [in][out] (layers.py:546-555)
        // k_conv_gn2 reads the weights fragment-major (after the packs above: the list runs in order)
        const int64_t w0f = (fuse && cout % 16 == 0) ? wres((int64_t)cout * K0a * 2) : -1, w1f = (fuse1 && cout % 16 == 0) ? wres((int64_t)cout * K1tot * 2) : -1;
        if (w0f >= 0) pack_frag(w0, w0f, cout, K0a, cin, 0);
        if (w1f >= 0) pack_frag(w1, w1f, cout, K1tot, cout, shortcut ? cin : 0);
        const int64_t b0 = pack_f32(p_c0b, cout), b1 = pack_f32(p_c1b, cout, shortcut ? p_c2b : -1);
        // time-embedding projection rows of this block inside the shared bank
        const int drow = dense_rows_next;
        pack_conv(p_dw, dense_w + (int64_t)drow * TEMB * 2, cout, TEMB, 1, TEMB, 0, TEMB);
        pack_f32_at(p_db, cout, dense_b + (int64_t)drow * 4);
        dense_rows_next += cout;

        const int64_t own_sc = arena.alloc((int64_t)std::max(cin, cout) * 4), own_sh = arena.alloc((int64_t)std::max(cin, cout) * 4);
        int64_t sc = own_sc, sh = own_sh;                 // GroupNorm_0's table: this block's buffers, or the one x's producer wrote
        emit_gn_stats(x, gn0, sc, sh, gn_mul);
        TRef h, xr;
        if (fold_up) {
            h = new_act(m.res, cin, 1);                   // activated, zero-bordered, at the INPUT resolution
            emit_gn_apply(x, sc, sh, h, nullptr, ACT_SILU, RS_NONE);
        } else if (!fuse) {
            h = new_act(ro, cin, 1);
            if (m.up || m.down) xr = new_act(ro, cin);
            emit_gn_apply(x, sc, sh, h, (m.up || m.down) ? &xr : nullptr, ACT_SILU, m.up ? RS_UP : (m.down ? RS_DOWN : RS_NONE));
        }

        // split-K workspace for the low-resolution levels (launch_gemm decides per launch): 4 slices of fp32 partial sums
        const int SK_MAX = 4;
        const int64_t skws = (ro <= 8) ? arena.alloc((int64_t)SK_MAX * ro * ro * cout * 4) : -1;
        TRef t = new_act(ro, cout);
        const Part pt = register_output(t, fuse);
        const int logW = ilog2(ro), logHW = 2 * logW, HWo = ro * ro;
        const int dtotal = dense_total; const int64_t dout = dense_out;
        op((fuse || fold_up) ? (ro <= 8 ? CLS_CONV_GN8 : CLS_CONV_GN) : CLS_GEMM, [=](const Ctx& c) {
            GemmArgs g = gemm_defaults();
            if (fold_up) {
                g.a0 = c.act(h); g.a0_ld = h.ld; g.a0_padded = 1; g.a0_C = cin; g.taps = 4; g.logW = logW - 1; g.logHW = logHW - 2;
                g.M = c.B * (HWo / 4); g.N = 4 * cout; g.b = c.w<bf16>(w0); g.b_ld = 4 * cin; g.bias_n = c.w<float>(b0);
                g.rowvec = c.at<float>(dout) + drow; g.rowvec_ld = dtotal; g.log_rows_per_sample = logHW - 2;
                g.c = c.act(t); g.c_ld = t.ld;
                if (pt.valid) { g.gn_part = c.at<float>(pt.off); g.gn_quads = pt.quads; }
                const int bm = launch_gemm(g, c.stream);
                if (pt.valid) c.part_bm[pt.id] = bm;
                return;
            }
            if (fuse) { g.a0 = c.act(x); g.a0_ld = x.ld; g.gn_scale = c.at<float>(sc); g.gn_shift = c.at<float>(sh); g.gn_ld = cin; g.gn_folded = 1; g.a0_up = fuse_up; }
            else { g.a0 = c.act(h); g.a0_ld = h.ld; g.a0_padded = 1; }
            g.a0_C = cin; g.taps = 9; g.logW = logW; g.logHW = logHW;
            g.M = c.B * HWo; g.N = cout; g.b = c.w<bf16>(w0); g.b_ld = K0a;
            if (w0f >= 0) g.b_frag = c.w<bf16>(w0f);
            g.bias_n = c.w<float>(b0);
            g.rowvec = c.at<float>(dout) + drow; g.rowvec_ld = dtotal; g.log_rows_per_sample = logHW;
            if (skws >= 0) { g.splitk_ws = c.at<float>(skws); g.splitk_max = SK_MAX; }
            g.c = c.act(t); g.c_ld = t.ld;
            if (pt.valid) { g.gn_part = c.at<float>(pt.off); g.gn_quads = pt.quads; set_fin(g, pt, c); }
            g_fin_written = false;
            const int bm = launch_gemm(g, c.stream);
            if (pt.valid) c.part_bm[pt.id] = bm;
            if (pt.fin && pt.fin->check) c.fin_done[pt.id] = g_fin_written;
        });
        if (!fuse) arena.release(h.off);
        int64_t sc1 = own_sc, sh1 = own_sh;               // GroupNorm_1's table: the same buffers again, or the one Conv_0's epilogue wrote
        emit_gn_stats(t, gn1, sc1, sh1, gn_mul1);
        TRef u;
        if (!fuse1) {
            u = new_act(ro, cout, 1);
            emit_gn_apply(t, sc1, sh1, u, nullptr, ACT_SILU, RS_NONE);
            arena.release(t.off);
        }
        if (pt.valid) arena.release(pt.off);
        const TRef xs = ((m.up || m.down) && !fuse_up) ? xr : x;           // shortcut source at the output resolution (fuse_up: x itself, fetched up-sampled)
        const float rs = res_scale;
        const Part po = register_output(out, fuse1);
        op(fuse1 ? (ro <= 8 ? CLS_CONV_GN8 : CLS_CONV_GN) : CLS_GEMM, [=](const Ctx& c) {
            GemmArgs g = gemm_defaults();
            if (fuse1) { g.a0 = c.act(t); g.a0_ld = t.ld; g.gn_scale = c.at<float>(sc1); g.gn_shift = c.at<float>(sh1); g.gn_ld = cout; g.gn_folded = 1; }
            else { g.a0 = c.act(u); g.a0_ld = u.ld; g.a0_padded = 1; }
            g.a0_C = cout; g.taps = 9; g.logW = logW; g.logHW = logHW;
            if (shortcut) { g.a1 = c.act(xs); g.a1_ld = xs.ld; g.a1_C = cin; g.a1_up = fuse_up; }
            else { g.resid = c.act(xs); g.resid_ld = xs.ld; }
            g.M = c.B * HWo; g.N = cout; g.b = c.w<bf16>(w1); g.b_ld = K1tot;
            if (w1f >= 0) g.b_frag = c.w<bf16>(w1f);
            g.bias_n = c.w<float>(b1); g.scale = rs;
            if (skws >= 0) { g.splitk_ws = c.at<float>(skws); g.splitk_max = SK_MAX; }
            g.c = c.act(out); g.c_ld = out.ld;
            if (po.valid) { g.gn_part = c.at<float>(po.off); g.gn_quads = po.quads; set_fin(g, po, c); }
            g_fin_written = false;
            const int bm = launch_gemm(g, c.stream);
            if (po.valid) c.part_bm[po.id] = bm;
            if (po.fin && po.fin->check) c.fin_done[po.id] = g_fin_written;
        });
        if (skws >= 0) arena.release(skws);
        if (fuse1) arena.release(t.off); else arena.release(u.off);
        if ((m.up || m.down) && !fuse_up) arena.release(xr.off);
        arena.release(own_sc); arena.release(own_sh);
        if (sc != own_sc) { arena.release(sc); arena.release(sh); }          // tables written by producers' epilogues: consumed
        if (sc1 != own_sc) { arena.release(sc1); arena.release(sh1); }
        E.taps[m.idx] = out;
    }

    void emit_attn(const Mod& m, const TRef& x, const TRef& out) {
        const int C = m.cin, T = m.res * m.res;
        const GN gn = take_gn(C);
        int64_t pw[4], pb[4];
        for (int i = 0; i < 4; ++i) { pw[i] = take((int64_t)C * C); pb[i] = take(C); }
        const int64_t wqk = wres((int64_t)2 * C * C * 2), wv = wres((int64_t)C * C * 2), w3 = wres((int64_t)C * C * 2);
        pack_transpose(pw[0], wqk, C, C, C);
        pack_transpose(pw[1], wqk + (int64_t)C * C * 2, C, C, C);
        pack_transpose(pw[2], wv, C, C, C);
        pack_transpose(pw[3], w3, C, C, C);
        const int64_t bqk = wres((int64_t)2 * C * 4);
        pack_f32_at(pb[0], C, bqk); pack_f32_at(pb[1], C, bqk + (int64_t)C * 4);
        const int64_t bv = pack_f32(pb[2], C), b3 = pack_f32(pb[3], C);

        const int64_t own_sc = arena.alloc((int64_t)C * 4), own_sh = arena.alloc((int64_t)C * 4);
        int64_t sc = own_sc, sh = own_sh;
        emit_gn_stats(x, gn, sc, sh);
        const bool fuse_qkv = T == 256 && C == 256 && g_attn_qkv;      // k_qkv256: x -> [q | k], V^T in one launch; h never exists
        TRef h = new_act(m.res, C);
        if (!fuse_qkv) emit_gn_apply(x, sc, sh, h, nullptr, ACT_NONE, RS_NONE);
        const int64_t qk = arena.alloc((int64_t)T * 2 * C * 2), vT = arena.alloc((int64_t)C * T * 2);
        // k_attn_blk256: projections, attention and output projection of a sample in ONE launch (needs the three fusions it is made of)
        const bool blk = fuse_qkv && g_attn_proj && g_attn_w8 && g_attn_blk;
        int64_t wqkvf = -1;
        const int64_t sc_q = sc, sh_q = sh;
        if (fuse_qkv) {
            wqkvf = wres((int64_t)3 * C * C * 2);
            const int64_t s0 = pw[0], s1 = pw[1], s2 = pw[2];
            E.packs.push_back([=](const PackCtx& p) { pack_attn_qkv_w(p.params + s0, p.params + s1, p.params + s2, reinterpret_cast<bf16*>(p.packed + wqkvf), p.stream); });
            const int64_t sc_ = sc, sh_ = sh;
            if (!blk)
            op(CLS_GEMM, [=](const Ctx& c) {
                if (g_record) return;
                AttnBlk256 a;
                a.B = c.B; a.x = c.act(x); a.x_ld = x.ld; a.sc = c.at<float>(sc_); a.sh = c.at<float>(sh_);
                a.wqkvf = c.w<bf16>(wqkvf); a.bqk = c.w<float>(bqk); a.bv = c.w<float>(bv); a.qk = c.at<bf16>(qk); a.vT = c.at<bf16>(vT);
                launch_attn_qkv256(a, c.stream);
            });
        }
        if (!fuse_qkv)
        op(CLS_GEMM, [=](const Ctx& c) {             // q | k  = h Wq | h Wk
            GemmArgs g = gemm_defaults();
            g.a0 = c.act(h); g.a0_ld = C; g.a0_C = C; g.M = c.B * T; g.N = 2 * C;
            g.b = c.w<bf16>(wqk); g.b_ld = C; g.bias_n = c.w<float>(bqk);
            g.c = c.at<bf16>(qk); g.c_ld = 2 * C;
            launch_gemm(g, c.stream);
        });
        if (!fuse_qkv)
        op(CLS_GEMM, [=](const Ctx& c) {             // V^T[b] = Wv^T h[b]^T  (so that P V is an "A B^T" product)
            GemmArgs g = gemm_defaults();
            g.a0 = c.w<bf16>(wv); g.a0_ld = C; g.a0_C = C; g.a_bs = 0; g.M = C; g.N = T;
            g.b = c.act(h); g.b_ld = C; g.b_bs = (int64_t)T * C; g.bias_m = c.w<float>(bv);
            g.c = c.at<bf16>(vT); g.c_ld = T; g.c_bs = (int64_t)C * T; g.batch = c.B;
            launch_gemm(g, c.stream);
        });
        arena.release(h.off);
        // k_attn256<true>: the output projection, skip connection and GroupNorm partials in the attention launch (attn256.h); O never exists
        const bool proj = T == 256 && C == 256 && g_attn_proj;
        int64_t w3f = -1;
        if (proj) {
            w3f = wres((int64_t)C * C * 2);
            const int64_t src = pw[3];
            E.packs.push_back([=](const PackCtx& p) { pack_attn_w3(p.params + src, reinterpret_cast<bf16*>(p.packed + w3f), p.stream); });
        }
        // k_attn_blk256_v2 (natinf_set_attn_block(2)): q k^T and P V against h itself -- the folded matrices Wqk = Wq Wk^T, Wvo = Wv W3 and their bias vectors, computed in
        // fp32 at load time (k_attn_fold_w) and packed like the q tiles / W3 of the four-projection plans
        const bool blk2 = blk && g_attn_blk == 2;
        int64_t wqf2 = -1, wvof2 = -1, cq2 = -1, bo2 = -1;
        if (blk2) {
            const int64_t fq = wres((int64_t)C * C * 4), fv = wres((int64_t)C * C * 4);
            cq2 = wres((int64_t)C * 4); bo2 = wres((int64_t)C * 4);
            wqf2 = wres((int64_t)C * C * 2); wvof2 = wres((int64_t)C * C * 2);
            const int64_t w0_ = pw[0], w1_ = pw[1], w2_ = pw[2], w3_ = pw[3], b0_ = pb[0], b2_ = pb[2], b3_ = pb[3], cq_ = cq2, bo_ = bo2, wq_ = wqf2, wv_ = wvof2;
            E.packs.push_back([=](const PackCtx& p) {
                pack_attn_fold(p.params + w0_, p.params + w1_, p.params + w2_, p.params + w3_, p.params + b0_, p.params + b2_, p.params + b3_,
                               reinterpret_cast<float*>(p.packed + fq), reinterpret_cast<float*>(p.packed + cq_), reinterpret_cast<float*>(p.packed + fv),
                               reinterpret_cast<float*>(p.packed + bo_), reinterpret_cast<bf16*>(p.packed + wq_), reinterpret_cast<bf16*>(p.packed + wv_), p.stream);
            });
        }
        const Part po_attn = proj ? register_output(out) : Part();
        const float rs_attn = res_scale;
        TRef O = new_act(m.res, C);
        if (T == 256 && C == 256) {
            // 16x16 attention: scores, softmax and P V of a sample in one block (attn_fused.h, two-phase: V^T follows K through LDS)
            op(CLS_GEMM, [=](const Ctx& c) {
                if (g_record) return;                    // natinf_ncsnpp_describe_gemms: GEMM launches only, nothing touches memory
                if (proj) {                              // the one-launch plans and k_attn256<true>: launch_attn_blk256, shared with natinf_debug_attn_block
                    AttnBlk256 a;
                    a.plan = blk2 ? 2 : (blk ? 1 : 0); a.B = c.B; a.x = c.act(x); a.x_ld = x.ld; a.sc = c.at<float>(sc_q); a.sh = c.at<float>(sh_q);
                    if (wqkvf >= 0) a.wqkvf = c.w<bf16>(wqkvf);
                    a.bqk = c.w<float>(bqk); a.bv = c.w<float>(bv); a.qk = c.at<bf16>(qk); a.vT = c.at<bf16>(vT); a.w3f = c.w<bf16>(w3f); a.b3 = c.w<float>(b3);
                    if (blk2) { a.wqf2 = c.w<bf16>(wqf2); a.cq2 = c.w<float>(cq2); a.wvof2 = c.w<bf16>(wvof2); a.bo2 = c.w<float>(bo2); }
                    a.out = c.act(out); a.o_ld = out.ld; a.out_scale = rs_attn;
                    if (po_attn.valid) { a.gn_part = c.at<float2>(po_attn.off); a.gn_quads = po_attn.quads; }
                    const int rows = launch_attn_blk256(a, c.stream);
                    if (po_attn.valid) c.part_bm[po_attn.id] = rows;
                }
                else
                    hipLaunchKernelGGL(k_attn256<false>, dim3((unsigned)(2 * c.B)), dim3(256), A256_LDS_BYTES, c.stream, c.at<bf16>(qk), 2 * C, C, c.at<bf16>(vT), c.act(O), C,
                                       1.0f / sqrtf((float)C), (const bf16*)nullptr, (const float*)nullptr, (const bf16*)nullptr, 0, 1.0f, (float2*)nullptr, 0);
            });
            arena.release(vT); arena.release(qk);
        } else {
        const int64_t S = arena.alloc((int64_t)T * T * 4);
            op(CLS_GEMM, [=](const Ctx& c) {             // S[b] = q[b] k[b]^T / sqrt(C)
                GemmArgs g = gemm_defaults();
                g.a0 = c.at<bf16>(qk); g.a0_ld = 2 * C; g.a0_C = C; g.a_bs = (int64_t)T * 2 * C; g.M = T; g.N = T;
                g.b = c.at<bf16>(qk) + C; g.b_ld = 2 * C; g.b_bs = (int64_t)T * 2 * C;
                g.scale = 1.0f / sqrtf((float)C);
                g.c = c.at<float>(S); g.c_ld = T; g.c_bs = (int64_t)T * T; g.c_mode = OUT_F32; g.batch = c.B;
                launch_gemm(g, c.stream);
            });
            const int64_t P = arena.alloc((int64_t)T * T * 2);
            op(CLS_OTHER, [=](const Ctx& c) {
                const int64_t rows = (int64_t)c.B * T;
                hipLaunchKernelGGL(k_softmax_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, c.stream,
                                   c.at<float>(S), c.at<bf16>(P), T, rows);
            });
            arena.release(S);
            op(CLS_GEMM, [=](const Ctx& c) {             // O[b] = P[b] V[b]
                GemmArgs g = gemm_defaults();
                g.a0 = c.at<bf16>(P); g.a0_ld = T; g.a0_C = T; g.a_bs = (int64_t)T * T; g.M = T; g.N = C;
                g.b = c.at<bf16>(vT); g.b_ld = T; g.b_bs = (int64_t)C * T;
                g.c = c.act(O); g.c_ld = C; g.c_bs = (int64_t)T * C; g.batch = c.B;
                launch_gemm(g, c.stream);
            });
            arena.release(P); arena.release(vT); arena.release(qk);
        }
        if (proj) {
            arena.release(O.off); arena.release(own_sc); arena.release(own_sh);
            if (sc != own_sc) { arena.release(sc); arena.release(sh); }
            E.taps[m.idx] = out;
            return;
        }
        const Part po = register_output(out);
        const float rs = res_scale;
        op(CLS_GEMM, [=](const Ctx& c) {             // out = (x + O W3 + b3) / sqrt(2)   (`ddpm`: no rescale)
            GemmArgs g = gemm_defaults();
            g.a0 = c.act(O); g.a0_ld = C; g.a0_C = C; g.M = c.B * T; g.N = C;
            g.b = c.w<bf16>(w3); g.b_ld = C; g.bias_n = c.w<float>(b3);
            g.resid = c.act(x); g.resid_ld = x.ld; g.scale = rs;
            g.c = c.act(out); g.c_ld = out.ld;
            if (po.valid) { g.gn_part = c.at<float>(po.off); g.gn_quads = po.quads; }
            const int bm = launch_gemm(g, c.stream);
            if (po.valid) c.part_bm[po.id] = bm;
        });
        arena.release(O.off); arena.release(own_sc); arena.release(own_sh);
        if (sc != own_sc) { arena.release(sc); arena.release(sh); }
        E.taps[m.idx] = out;
    }

    // ---- `ddpm` resampling modules (layers.py:586-612) ------------------------------------------------
    // Downsample: 3x3 convolution, stride 2, 'SAME' padding emulated by one zero row / column at the bottom / right.  Three launches per
    // forward: an im2col pass (k_inc_im2col, K order tap-major) + one GEMM of the shared tile family.
    void emit_downconv(const Mod& m, const TRef& x, const TRef& out) {
        const int C = m.cin, ro = m.res / 2, Kd = 9 * C;
        const int64_t pw = take((int64_t)C * C * 9), pb = take(C);
        const int64_t w = wres((int64_t)C * Kd * 2);
        E.packs.push_back([=](const PackCtx& p) {              // k = tap * C + c (the im2col order)
            const int64_t n = (int64_t)C * C * 9;
            hipLaunchKernelGGL(k_pack_conv, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream, p.params + pw, reinterpret_cast<bf16*>(p.packed + w), C, C, 9, Kd, 0, C, 0, 1.0f);
        });
        const int64_t b = pack_f32(pb, C);
        const int64_t col = arena.alloc((int64_t)ro * ro * Kd * 2);
        const Part po = register_output(out);
        const int rin = m.res;
        op(CLS_GEMM, [=](const Ctx& c) {
            const int64_t M = (int64_t)c.B * ro * ro;
            if (!g_record) {
                const int64_t total = M * (Kd / 8);
                hipLaunchKernelGGL(k_inc_im2col, dim3(grid1d(total, 256, 1 << 30)), dim3(256), 0, c.stream, c.act(x), rin, rin, x.ld, C, 3, 3, 2, 0, 0, ro, ro, Kd,
                                   c.at<bf16>(col), total);
            }
            GemmArgs g = gemm_defaults();
            g.a0 = c.at<bf16>(col); g.a0_ld = Kd; g.a0_C = Kd; g.M = (int)M; g.N = C; g.b = c.w<bf16>(w); g.b_ld = Kd; g.bias_n = c.w<float>(b);
            g.log_rows_per_sample = 2 * ilog2(ro); g.logHW = 2 * ilog2(ro); g.logW = ilog2(ro);
            g.c = c.act(out); g.c_ld = out.ld;
            if (po.valid) { g.gn_part = c.at<float>(po.off); g.gn_quads = po.quads; }
            const int bm = launch_gemm(g, c.stream);
            if (po.valid) c.part_bm[po.id] = bm;
        });
        arena.release(col);
        E.taps[m.idx] = out;
    }
    // Upsample: nearest 2x, then a 3x3 convolution: the resampling pass (identity scale / shift, no activation) writes the zero-bordered
    // up-sampled copy the implicit GEMM reads
    int64_t ident_sc = -1, ident_sh = -1;
    void emit_upconv(const Mod& m, const TRef& x, const TRef& out) {
        const int C = m.cin, ro = m.res * 2, Ku = 9 * C;
        const int64_t pw = take((int64_t)C * C * 9), pb = take(C);
        const int64_t w = wres((int64_t)C * Ku * 2);
        pack_conv(pw, w, C, C, 9, Ku, 0, C);
        const int64_t b = pack_f32(pb, C);
        if (ident_sc < 0) {                                   // per (sample, channel) scale 1 / shift 0, filled once per forward
            ident_sc = arena.alloc((int64_t)2 * NF * 4); ident_sh = arena.alloc((int64_t)2 * NF * 4);
            const int64_t isc = ident_sc, ish = ident_sh;
            op(CLS_OTHER, [=](const Ctx& c) {
                const int64_t n = (int64_t)c.B * 2 * NF;
                hipLaunchKernelGGL(k_fill_f32, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, c.stream, c.at<float>(isc), 1.0f, n);
                hipLaunchKernelGGL(k_fill_f32, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, c.stream, c.at<float>(ish), 0.0f, n);
            });
        }
        TRef u = new_act(ro, C, 1);
        emit_gn_apply(x, ident_sc, ident_sh, u, nullptr, ACT_NONE, RS_UP);
        const Part po = register_output(out);
        const int logW = ilog2(ro);
        op(CLS_GEMM, [=](const Ctx& c) {
            GemmArgs g = gemm_defaults();
            g.a0 = c.act(u); g.a0_ld = u.ld; g.a0_C = C; g.taps = 9; g.logW = logW; g.logHW = 2 * logW; g.a0_padded = 1;
            g.M = c.B * ro * ro; g.N = C; g.b = c.w<bf16>(w); g.b_ld = Ku; g.bias_n = c.w<float>(b); g.log_rows_per_sample = 2 * logW;
            g.c = c.act(out); g.c_ld = out.ld;
            if (po.valid) { g.gn_part = c.at<float>(po.off); g.gn_quads = po.quads; }
            const int bm = launch_gemm(g, c.stream);
            if (po.valid) c.part_bm[po.id] = bm;
        });
        arena.release(u.off);
        E.taps[m.idx] = out;
    }

    int dense_rows_next = 0;

    // ---- fused GroupNorm statistics: partial tables written by GEMM epilogues ------------------------
    // Fin: the producer's epilogue writes its consumer's GroupNorm table (GemmArgs::fin_*).  The table buffers are allocated with the Part -- in front
    // of the producing launch, so they cannot alias anything that launch still reads -- and the consumer fills in its gamma / beta when it is emitted
    // (the producer's op reads the struct when it RUNS).  Only the first single-source consumer claims it; anyone else takes k_gn_finalize.
    // check (round 5, the 16x16 level): whether the producer's launch wrote the table is only known when it RUNS (k_conv_gn3's 256 x 256 tile does, the k_conv_gn2 tiles a
    // tuning knob may select instead do not): the producer's op records it in Ctx::fin_done (per forward), and the consumer's op launches k_gn_finalize into the same buffers when it is false
    struct Fin { int64_t sc = -1, sh = -1, gamma = -1, beta = -1; int C = 0; float out_mul = 1.0f; bool claimed = false, check = false; };
    struct Part { int64_t off = -1; int quads = 0, id = -1, res = 0; bool valid = false; std::shared_ptr<Fin> fin; };
    static void set_fin(GemmArgs& g, const Part& p, const Ctx& c) {
        if (!p.fin || !p.fin->claimed) return;
        const Fin& f = *p.fin;
        g.fin_scale = c.at<float>(f.sc); g.fin_shift = c.at<float>(f.sh); g.fin_gamma = c.w<float>(f.gamma); g.fin_beta = c.w<float>(f.beta);
        g.fin_ld = f.C; g.fin_cg = f.C / 32; g.fin_mul = f.out_mul; g.fin_eps = GN_EPS;
    }
    std::map<std::pair<int64_t, int>, Part> parts;      // (tensor offset, channel offset) -> latest producer's table
    int n_parts = 0;
    static bool fusable(int res) { return res >= 16; }   // every block tile (<= 256 rows) lies inside one sample
    Part new_part(int res, int C) {
        Part p; p.quads = C / 4; p.res = res; p.id = n_parts++; p.valid = true;
        p.off = arena.alloc((int64_t)std::max(res * res / 64, 1) * p.quads * 8);       // worst case: 64-row block tiles (4x4: one row per sample)
        return p;
    }
    // called for EVERY module output so that a stale table can never be matched to a later tensor at the same place
    // fused8: the producer is the fused convolution at 8x8, whose epilogue writes one partial row per SAMPLE (two per tile); any other producer's
    // 128-row tiles span two 8x8 samples, and its consumers take the streaming statistics kernel
    Part register_output(const TRef& out, bool fused8 = false) {
        Part p;
        if (fusable(out.res) || (out.res <= 8 && fused8)) p = new_part(out.res, out.C);
        if (p.valid && out.res <= 8 && fused8 && (g_fuse_fin & 1) && out.C == 256) {      // (the fused kernel's 64-pixel x 256-channel tile: whole samples, every channel)
            p.fin = std::make_shared<Fin>();
            p.fin->sc = arena.alloc((int64_t)out.C * 4); p.fin->sh = arena.alloc((int64_t)out.C * 4); p.fin->C = out.C;
        }
        // 16x16 (round 5): k_conv_gn3's 256 x 256 tile = ONE sample x every channel (fused8 here: "the producer is the fused convolution")
        if (p.valid && out.res == 16 && fused8 && (g_fuse_fin & 2) && out.C == 256 && !ddpm) {
            p.fin = std::make_shared<Fin>();
            p.fin->sc = arena.alloc((int64_t)out.C * 4); p.fin->sh = arena.alloc((int64_t)out.C * 4); p.fin->C = out.C; p.fin->check = true;
        }
        parts[{out.off, out.coff}] = p;
        return p;
    }
    // statistics of x from partial tables if every channel slice of x has a valid one; otherwise the streaming kernel.
    // (Folding the tables inside k_gn_apply instead of this one-block-per-sample launch was built and measured: bit-identical,
    // 1.6 % SLOWER per forward in a same-box A/B -- every 4-row apply block then starts with two dependent load round trips.)
    bool emit_gn_from_parts(const TRef& x, GN gn, int64_t& sc, int64_t& sh, float out_mul) {
        std::vector<Part> src;
        int ch = 0;
        while (ch < x.C) {
            auto it = parts.find({x.off, x.coff + ch});
            if (it == parts.end() || !it->second.valid || it->second.res != x.res) return false;
            src.push_back(it->second);
            ch += it->second.quads * 4;
        }
        if (ch != x.C || src.empty() || src.size() > 2) return false;
        const Part p0 = src[0], p1 = src.size() > 1 ? src[1] : Part();
        const int HW = x.res * x.res, C = x.C;
        if (src.size() == 1 && p0.fin && !p0.fin->claimed && p0.fin->C == C) {          // the producer's epilogue writes this table: no launch
            Fin& f = *p0.fin;
            f.gamma = gn.gamma; f.beta = gn.beta; f.out_mul = out_mul; f.claimed = true;
            sc = f.sc; sh = f.sh;
            if (f.check) {                                                              // ... unless the launch that ran was not the one that can (see Fin)
                const std::shared_ptr<Fin> fp = p0.fin;
                const int64_t fsc = f.sc, fsh = f.sh;
                op(CLS_OTHER, [=](const Ctx& c) {
                    if (c.fin_done[p0.id]) return;
                    hipLaunchKernelGGL(k_gn_finalize, dim3(c.B), dim3(256), 0, c.stream, c.at<float2>(p0.off), HW / c.part_bm[p0.id], p0.quads, (const float2*)nullptr, 0, 0, C, HW,
                                       c.w<float>(gn.gamma), c.w<float>(gn.beta), c.at<float>(fsc), c.at<float>(fsh), GN_EPS, out_mul);
                });
            }
            return true;
        }
        const int64_t sc_ = sc, sh_ = sh;
        op(CLS_OTHER, [=](const Ctx& c) {
            const int tps0 = HW / c.part_bm[p0.id], tps1 = p1.valid ? HW / c.part_bm[p1.id] : 0;
            hipLaunchKernelGGL(k_gn_finalize, dim3(c.B), dim3(256), 0, c.stream, c.at<float2>(p0.off), tps0, p0.quads,
                               p1.valid ? c.at<float2>(p1.off) : (const float2*)nullptr, tps1, p1.valid ? p1.quads : 0, C, HW,
                               c.w<float>(gn.gamma), c.w<float>(gn.beta), c.at<float>(sc_), c.at<float>(sh_), GN_EPS, out_mul);
        });
        return true;
    }

    // ---- module list (ncsnpp.py:66-230) ----------------------------------------------------
    void list_modules() {
        auto add = [&](int kind, int cin, int cout, int up, int down, int res) {
            Mod m; m.idx = (int)E.mods.size(); m.kind = kind; m.cin = cin; m.cout = cout; m.up = up; m.down = down; m.res = res; m.poff = 0;
            E.mods.push_back(m);
        };
        add(K_LIN, NF, TEMB, 0, 0, 0); add(K_LIN, TEMB, TEMB, 0, 0, 0); add(K_CONV, 3, NF, 0, 0, IMG);
        std::vector<int> skip = {NF};
        int ch = NF, res = IMG;
        for (int l = 0; l < NLEVEL; ++l) {
            for (int b = 0; b < NUM_RES; ++b) {
                add(K_RES, ch, NF * CH_MULT[l], 0, 0, res); ch = NF * CH_MULT[l];
                if (attn_at(res)) add(K_ATTN, ch, ch, 0, 0, res);
                skip.push_back(ch);
            }
            if (l != NLEVEL - 1) { if (ddpm) add(K_DOWN, ch, ch, 0, 0, res); else add(K_RES, ch, ch, 0, 1, res); res /= 2; skip.push_back(ch); }
        }
        add(K_RES, ch, ch, 0, 0, res); add(K_ATTN, ch, ch, 0, 0, res); add(K_RES, ch, ch, 0, 0, res);
        for (int l = NLEVEL - 1; l >= 0; --l) {
            for (int b = 0; b < NUM_RES + 1; ++b) { add(K_RES, ch + skip.back(), NF * CH_MULT[l], 0, 0, res); skip.pop_back(); ch = NF * CH_MULT[l]; }
            if (attn_at(res)) add(K_ATTN, ch, ch, 0, 0, res);
            if (l != 0) { if (ddpm) add(K_UP, ch, ch, 0, 0, res); else add(K_RES, ch, ch, 1, 0, res); res *= 2; }
        }
        add(K_GN, ch, ch, 0, 0, res); add(K_CONV, ch, 3, 0, 0, res);
    }

    void build() {
        list_modules();
        auto& M = E.mods;
        // ---- the U-Net's concat buffers: up-path res-block j reads cat([h, skip]) --------------
        struct Cat { TRef buf; int ch_h, ch_s; };
        std::vector<Cat> cats;
        std::vector<int> skip_ch, skip_res;
        {   // dry walk to size them
            int ch = NF, res = IMG; skip_ch.push_back(NF); skip_res.push_back(IMG);
            for (int l = 0; l < NLEVEL; ++l) {
                for (int b = 0; b < NUM_RES; ++b) { ch = NF * CH_MULT[l]; skip_ch.push_back(ch); skip_res.push_back(res); }
                if (l != NLEVEL - 1) { res /= 2; skip_ch.push_back(ch); skip_res.push_back(res); }
            }
            int sp = (int)skip_ch.size();
            for (int l = NLEVEL - 1; l >= 0; --l) {
                for (int b = 0; b < NUM_RES + 1; ++b) {
                    --sp;
                    Cat c; c.ch_h = ch; c.ch_s = skip_ch[sp];
                    c.buf = new_act(res, c.ch_h + c.ch_s);
                    cats.push_back(c);
                    ch = NF * CH_MULT[l];
                }
                if (l != 0) res *= 2;
            }
        }
        const int P = (int)skip_ch.size();
        auto skip_slot = [&](int i) { const Cat& c = cats[P - 1 - i]; TRef t = c.buf; t.C = c.ch_s; t.coff = c.ch_h; return t; };
        auto h_slot = [&](int j) { const Cat& c = cats[j]; TRef t = c.buf; t.C = c.ch_h; t.coff = 0; return t; };

        // ---- shared time-embedding bank -------------------------------------------------------
        for (auto& m : M) if (m.kind == K_RES) dense_total += m.cout;
        dense_w = wres((int64_t)dense_total * TEMB * 2); dense_b = wres((int64_t)dense_total * 4);
        dense_out = arena.alloc((int64_t)dense_total * 4);
        const int64_t emb = arena.alloc(128 * 2), t1 = arena.alloc(TEMB * 2), t2 = arena.alloc(TEMB * 2);

        size_t mi = 0;
        // modules 0, 1: Linear(128,512), Linear(512,512)
        {
            const Mod& m0 = M[mi++]; const Mod& m1 = M[mi++]; (void)m0; (void)m1;
            const int64_t pw0 = take((int64_t)TEMB * NF), pb0 = take(TEMB), pw1 = take((int64_t)TEMB * TEMB), pb1 = take(TEMB);
            const int64_t w0 = wres((int64_t)TEMB * NF * 2), w1 = wres((int64_t)TEMB * TEMB * 2);
            pack_conv(pw0, w0, TEMB, NF, 1, NF, 0, NF); pack_conv(pw1, w1, TEMB, TEMB, 1, TEMB, 0, TEMB);
            const int64_t b0 = pack_f32(pb0, TEMB), b1 = pack_f32(pb1, TEMB);
            const int64_t dw = dense_w, db = dense_b, dout = dense_out; const int dtot = dense_total;
            op(CLS_OTHER, [=](const Ctx& c) {
                // one thread per element and no grid stride: the grid must cover B * 128 (grid1d's default cap of 4096 blocks left samples 8192.. unwritten)
                hipLaunchKernelGGL(k_time_embed, dim3(grid1d((int64_t)c.B * 128, 256, 1 << 30)), dim3(256), 0, c.stream, c.labels, c.at<bf16>(emb), c.B);
            });
            op(CLS_GEMM, [=](const Ctx& c) {
                GemmArgs g = gemm_defaults();                        // act(Linear_0(emb))
                g.a0 = c.at<bf16>(emb); g.a0_ld = NF; g.a0_C = NF; g.M = c.B; g.N = TEMB;
                g.b = c.w<bf16>(w0); g.b_ld = NF; g.bias_n = c.w<float>(b0); g.act = ACT_SILU;
                g.c = c.at<bf16>(t1); g.c_ld = TEMB;
                launch_gemm(g, c.stream);
                g = gemm_defaults();                                 // act(temb) = act(Linear_1(.))
                g.a0 = c.at<bf16>(t1); g.a0_ld = TEMB; g.a0_C = TEMB; g.M = c.B; g.N = TEMB;
                g.b = c.w<bf16>(w1); g.b_ld = TEMB; g.bias_n = c.w<float>(b1); g.act = ACT_SILU;
                g.c = c.at<bf16>(t2); g.c_ld = TEMB;
                launch_gemm(g, c.stream);
                g = gemm_defaults();                                 // every block's Dense_0(act(temb)) at once
                g.a0 = c.at<bf16>(t2); g.a0_ld = TEMB; g.a0_C = TEMB; g.M = c.B; g.N = dtot;
                g.b = c.w<bf16>(dw); g.b_ld = TEMB; g.bias_n = c.w<float>(db);
                g.c = c.at<float>(dout); g.c_ld = dtot; g.c_mode = OUT_F32;
                launch_gemm(g, c.stream);
            });
        }
        // module 2: stem conv 3 -> 128 as im2col (K padded 27 -> 64) + GEMM
        int si = 0;
        TRef cur = skip_slot(si++);
        {
            const Mod& m = M[mi++];
            const int64_t pw = take((int64_t)NF * 27), pb = take(NF);
            const int64_t w = wres((int64_t)NF * 64 * 2);
            pack_zero(w, (int64_t)NF * 64);
            pack_conv(pw, w, NF, 3, 9, 64, 0, 3);
            const int64_t b = pack_f32(pb, NF);
            const int64_t a0 = arena.alloc((int64_t)IMG * IMG * 64 * 2);
            const TRef dst = cur;
            const Part po = register_output(dst);
            op(CLS_OTHER, [=](const Ctx& c) {
                const int64_t rows = (int64_t)c.B * IMG * IMG;
                hipLaunchKernelGGL(k_stem_im2col, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, c.stream, c.x, c.at<bf16>(a0), rows);
            });
            op(CLS_GEMM, [=](const Ctx& c) {
                const int64_t rows = (int64_t)c.B * IMG * IMG;
                GemmArgs g = gemm_defaults();
                g.a0 = c.at<bf16>(a0); g.a0_ld = 64; g.a0_C = 64; g.M = (int)rows; g.N = NF;
                g.b = c.w<bf16>(w); g.b_ld = 64; g.bias_n = c.w<float>(b);
                g.c = c.act(dst); g.c_ld = dst.ld;
                if (po.valid) { g.gn_part = c.at<float>(po.off); g.gn_quads = po.quads; }
                const int bm = launch_gemm(g, c.stream);
                if (po.valid) c.part_bm[po.id] = bm;
            });
            arena.release(a0);
            E.taps[m.idx] = dst;
        }
        // ---- down path ------------------------------------------------------------------------
        int res = IMG;
        for (int l = 0; l < NLEVEL; ++l) {
            for (int b = 0; b < NUM_RES; ++b) {
                const Mod& m = M[mi++];
                const TRef dst = skip_slot(si++);
                if (attn_at(res)) {
                    TRef tmp = new_act(res, m.cout);
                    emit_res(m, cur, tmp);
                    emit_attn(M[mi++], tmp, dst);
                    arena.release(tmp.off);
                } else {
                    emit_res(m, cur, dst);
                }
                cur = dst;
            }
            if (l != NLEVEL - 1) {
                const Mod& m = M[mi++];
                const TRef dst = skip_slot(si++);
                if (ddpm) emit_downconv(m, cur, dst); else emit_res(m, cur, dst);
                cur = dst; res /= 2;
            }
        }
        // ---- middle ---------------------------------------------------------------------------
        {
            TRef a = new_act(res, cur.C), b = new_act(res, cur.C);
            emit_res(M[mi++], cur, a);
            emit_attn(M[mi++], a, b);
            arena.release(a.off);
            emit_res(M[mi++], b, h_slot(0));
            arena.release(b.off);
        }
        // ---- up path --------------------------------------------------------------------------
        int j = 0;
        TRef last;
        for (int l = NLEVEL - 1; l >= 0; --l) {
            for (int b = 0; b < NUM_RES + 1; ++b) {
                const Mod& m = M[mi++];
                const bool level_end = b == NUM_RES;
                TRef in = cats[j].buf;                           // cat([h, skip]) along channels
                TRef dst = level_end ? new_act(res, m.cout) : h_slot(j + 1);
                emit_res(m, in, dst);
                arena.release(cats[j].buf.off);
                last = dst; ++j;
            }
            if (attn_at(res)) {
                TRef dst = new_act(res, last.C);
                emit_attn(M[mi++], last, dst);
                arena.release(last.off);
                last = dst;
            }
            if (l != 0) {
                const Mod& m = M[mi++];
                if (ddpm) emit_upconv(m, last, h_slot(j)); else emit_res(m, last, h_slot(j));
                arena.release(last.off);
                res *= 2;
            }
        }
        // ---- head: GroupNorm -> SiLU -> conv3x3 128 -> 3, written as fp32 NCHW -----------------
        {
            const Mod& mg = M[mi++]; const Mod& mc = M[mi++];
            const GN gn = take_gn(mg.cin);
            const int64_t pw = take((int64_t)3 * mc.cin * 9), pb = take(3);
            const int Kf = 9 * mc.cin;
            const int64_t w = wres((int64_t)3 * Kf * 2);
            pack_conv(pw, w, 3, mc.cin, 9, Kf, 0, mc.cin);
            const int64_t b = pack_f32(pb, 3);
            int64_t sc = arena.alloc((int64_t)mg.cin * 4), sh = arena.alloc((int64_t)mg.cin * 4);          // (32x32: never a producer-written table)
            const int logW = ilog2(res), cinf = mc.cin;
            if (g_fuse_head && res == HeadConvCfg::RES && mc.cin == HeadConvCfg::C) {
                // one launch (head_conv.h): raw tensor in, fp32 NCHW out; folded GroupNorm form (scale / shift x -log2 e, weights x -ln 2)
                const int64_t w16 = wres((int64_t)16 * Kf * 2);
                pack_zero(w16, (int64_t)16 * Kf);
                pack_conv(pw, w16, 3, mc.cin, 9, Kf, 0, mc.cin, -0.6931471805599453f);
                emit_gn_stats(last, gn, sc, sh, -1.4426950408889634f);
                const TRef src = last;
                op(CLS_GEMM, [=](const Ctx& c) {
                    if (g_record) { *g_record += gemm_row(c.B * res * res, 3, Kf, 0, 9, 1, "head_conv", 0) + "\n"; return; }
                    hipLaunchKernelGGL(k_head_conv, dim3((unsigned)(c.B * (HeadConvCfg::RES / HeadConvCfg::ROWS))), dim3(256), HeadConvCfg::LDS_BYTES, c.stream,
                                       c.act(src), src.ld, c.at<float>(sc), c.at<float>(sh), c.w<bf16>(w16), c.w<float>(b), c.out);
                });
            } else {
            emit_gn_stats(last, gn, sc, sh);
            TRef u = new_act(res, mg.cin, 1);
            emit_gn_apply(last, sc, sh, u, nullptr, ACT_SILU, RS_NONE);
            op(CLS_GEMM, [=](const Ctx& c) {
                GemmArgs g = gemm_defaults();
                g.a0 = c.act(u); g.a0_ld = u.ld; g.a0_C = cinf; g.taps = 9; g.logW = logW; g.logHW = 2 * logW; g.a0_padded = 1;
                g.M = c.B * res * res; g.N = 3; g.b = c.w<bf16>(w); g.b_ld = Kf; g.bias_n = c.w<float>(b);
                g.c = c.out; g.c_mode = OUT_F32_NCHW;
                launch_gemm(g, c.stream);
            });
            }
            E.taps[mg.idx] = last;          // (pre-norm tensor; the GN module's own output is internal)
        }
        finish();
        E.part_bm.assign(n_parts > 0 ? n_parts : 1, 128);
        E.fin_done.assign(n_parts > 0 ? n_parts : 1, 0);
        // parameter offsets for describe(): recompute by module in order
    }
};

int64_t module_param_count(const Mod& m) {
    switch (m.kind) {
        case K_LIN: return (int64_t)m.cout * m.cin + m.cout;
        case K_CONV: return (int64_t)m.cout * m.cin * 9 + m.cout;
        case K_GN: return 2 * (int64_t)m.cin;
        case K_DOWN: case K_UP: return (int64_t)m.cout * m.cin * 9 + m.cout;
        case K_ATTN: return 2 * (int64_t)m.cin + 4 * ((int64_t)m.cin * m.cin + m.cin);
        case K_RES: {
            int64_t n = 2 * (int64_t)m.cin + (int64_t)m.cout * m.cin * 9 + m.cout + (int64_t)m.cout * TEMB + m.cout +
                        2 * (int64_t)m.cout + (int64_t)m.cout * m.cout * 9 + m.cout;
            if (m.cin != m.cout || m.up || m.down) n += (int64_t)m.cout * m.cin + m.cout;
            return n;
        }
    }
    return 0;
}

natinf_ncsnpp* make_engine(int flags) {
    natinf_ncsnpp* e = new natinf_ncsnpp();
    e->flags = flags;
    Builder b(*e);
    b.build();
    int64_t off = 0;
    for (auto& m : e->mods) { m.poff = off; off += module_param_count(m); }
    if (off != e->n_params) { delete e; return nullptr; }      // plan and parameter walk disagree
    return e;
}

// The size queries without a handle answer for the LARGEST plan (every build-time fusion on: each adds repacked weight copies), whatever the
// A/B knobs are set to when they are first asked -- a packed buffer of that size fits every plan.
const natinf_ncsnpp& reference_engine() {
    static natinf_ncsnpp* e = [] {
        // every knob that is read when a plan is BUILT and adds a repacked weight copy or a table: saved, forced on, restored
        int* knobs[] = {&g_fuse_gn, &g_fuse_up, &g_fuse_head, &g_fuse_gn8, &g_fuse_gn4, &g_fuse_fin, &g_attn_qkv, &g_attn_proj};
        int saved[sizeof(knobs) / sizeof(knobs[0])];
        for (size_t i = 0; i < sizeof(knobs) / sizeof(knobs[0]); ++i) { saved[i] = *knobs[i]; *knobs[i] = 1; }
        g_fuse_fin = 3;                                      // (a bit mask: both levels' producer-written tables)
        const int saved_fold = g_fuse_up_fold;
        g_fuse_up_fold = 0;                                  // (the folded 2x2 kernels, 16 cin cout, REPLACE the packed and the fragment-major nine-tap copies, 18 cin cout: off is the larger plan)
        natinf_ncsnpp* r = make_engine(0);
        g_fuse_up_fold = saved_fold;
        for (size_t i = 0; i < sizeof(knobs) / sizeof(knobs[0]); ++i) *knobs[i] = saved[i];
        return r;
    }();
    return *e;
}

}  // namespace

extern "C" {

int64_t natinf_ncsnpp_param_count(void) { return reference_engine().n_params; }
int64_t natinf_ncsnpp_packed_bytes(void) { return reference_engine().packed_bytes; }

int64_t natinf_ncsnpp_handle_param_count(natinf_ncsnpp_t h) { return h ? h->n_params : NATINF_EINVAL; }
int64_t natinf_ncsnpp_handle_packed_bytes(natinf_ncsnpp_t h) { return h ? h->packed_bytes : NATINF_EINVAL; }

int64_t natinf_ncsnpp_workspace_bytes(natinf_ncsnpp_t h, int max_batch) {
    if (!h || max_batch <= 0) return NATINF_EINVAL;
    return h->ws_per_image * (int64_t)max_batch;
}

// every switch a plan builder reads (layout of the packed weights included), one byte each
static uint64_t plan_signature() {
    const int k[] = {g_fuse_head, g_attn_qkv, g_attn_w8, g_attn_proj, g_fuse_gn8, g_fuse_fin, g_fuse_gn4, g_fuse_gn, g_cg_wide, g_fuse_up,
                     g_attn_blk /* (2: the folded attention weights are packed too) */, g_fuse_up_fold, g_cg3 /* read by the plan builders (which launches exist; which tables a producer may write) */};
    uint64_t h = 1469598103934665603ull;
    for (int v : k) h = (h ^ (uint64_t)(v & 0xff)) * 1099511628211ull;
    return h;
}

int natinf_ncsnpp_create(natinf_ncsnpp_t* out, int flags) {
    if (!out || (flags & ~(NATINF_NCSNPP_KEEP_ACTIVATIONS | NATINF_NCSNPP_DDPM))) return NATINF_EINVAL;
    natinf_ncsnpp* e = make_engine(flags);
    if (!e) return NATINF_ESTATE;
    e->plan_sig = plan_signature();
    *out = e;
    return NATINF_OK;
}

int natinf_ncsnpp_destroy(natinf_ncsnpp_t h) {
    if (!h) return NATINF_EINVAL;
    for (auto& r : h->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : h->pool) (void)hipEventDestroy(e);
    delete h;
    return NATINF_OK;
}

int natinf_ncsnpp_describe(natinf_ncsnpp_t h, char* buf, int cap) {
    if (!h || !buf || cap <= 0) return NATINF_EINVAL;
    std::string s;
    char line[160];
    for (const auto& m : h->mods) {
        snprintf(line, sizeof(line), "%d %s %d %d %d %d %d %lld\n", m.idx, kind_name(m.kind), m.cin, m.cout, m.up, m.down, m.res,
                 (long long)m.poff);
        s += line;
    }
    if ((int)s.size() + 1 > cap) return NATINF_EINVAL;
    memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
}

int natinf_ncsnpp_load(natinf_ncsnpp_t h, const float* params_f32, int64_t n_params, void* packed, int64_t packed_bytes,
                       natinf_stream_t stream) {
    return h ? h->load(params_f32, n_params, packed, packed_bytes, (hipStream_t)stream) : NATINF_EINVAL;
}

int natinf_ncsnpp_share(natinf_ncsnpp_t h, natinf_ncsnpp_t loaded) {
    if (!h || !loaded || h == loaded) return NATINF_EINVAL;
    if (!loaded->packed) return NATINF_ESTATE;
    // same network, same plan-build-time switches: the two plans address the packed buffer identically
    if ((h->flags & NATINF_NCSNPP_DDPM) != (loaded->flags & NATINF_NCSNPP_DDPM) || h->n_params != loaded->n_params || h->packed_bytes != loaded->packed_bytes ||
        h->packs.size() != loaded->packs.size() || h->plan_sig != loaded->plan_sig)
        return NATINF_EINVAL;
    h->packed = loaded->packed;
    return NATINF_OK;
}

int natinf_ncsnpp_forward(natinf_ncsnpp_t h, const float* x, const float* labels, float* out, int B, void* workspace,
                          int64_t workspace_bytes, natinf_stream_t stream) {
    if (!h || !x || !labels || !out || !workspace || B <= 0) return NATINF_EINVAL;
    if (!h->packed) return NATINF_ESTATE;
    if (workspace_bytes < h->ws_per_image * (int64_t)B || (int64_t)B * IMG * IMG >= (1LL << 31)) return NATINF_EINVAL;
    if (!h->configured) {
        if (!configure_gemm_kernels()) return NATINF_ENODEV;
        h->configured = true;
    }
    Ctx c{B, reinterpret_cast<unsigned char*>(workspace), h->packed, (hipStream_t)stream, x, labels, out, h->part_bm.data()};
    c.fin_done = h->fin_done.data();
    g_launch_error = 0;
    if (!h->prof) {
        for (const auto& f : h->ops) f(c);
    } else {
        for (size_t i = 0; i < h->ops.size(); ++i) {
            natinf_ncsnpp::Rec r; r.cls = h->op_cls[i];
            for (hipEvent_t* e : {&r.a, &r.b}) {
                if (!h->pool.empty()) { *e = h->pool.back(); h->pool.pop_back(); }
                else if (hipEventCreate(e) != hipSuccess) return NATINF_ELAUNCH;
            }
            (void)hipEventRecord(r.a, c.stream);
            h->ops[i](c);
            (void)hipEventRecord(r.b, c.stream);
            h->recs.push_back(r);
        }
    }
    h->last_B = B; h->last_ws = c.ws;
    if (g_launch_error) { g_launch_error = 0; return NATINF_ESTATE; }
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_ncsnpp_describe_gemms(natinf_ncsnpp_t h, int B, char* buf, int cap) {
    if (!h || !buf || cap <= 0 || B <= 0) return NATINF_EINVAL;
    std::string out;
    g_record = &out;
    std::vector<int> scratch_bm(h->part_bm.size(), 128);
    // (a non-null fake workspace base: launches are only described, but "is this pointer set" decides the kernel variant)
    std::vector<unsigned char> scratch_done(h->part_bm.size(), 0);
    Ctx c{B, reinterpret_cast<unsigned char*>(4096), reinterpret_cast<const unsigned char*>(4096), nullptr, nullptr, nullptr, nullptr, scratch_bm.data()};
    c.fin_done = scratch_done.data();
    for (size_t i = 0; i < h->ops.size(); ++i)
        if (h->op_cls[i] == CLS_GEMM || h->op_cls[i] == CLS_CONV_GN || h->op_cls[i] == CLS_CONV_GN8) h->ops[i](c);          // GEMM ops only compute pointers and call launch_gemm
    g_record = nullptr;
    if ((int)out.size() + 1 > cap) return NATINF_EINVAL;
    memcpy(buf, out.c_str(), out.size() + 1);
    return (int)out.size();
}

int natinf_debug_gemm(int variant, int M, int N, int K0, int K1, int taps, int logW, int batch,
                      const void* a0, const void* a1, const void* b, const float* bias_n, void* c, int c_f32, float scale,
                      int iters, natinf_stream_t stream) {
    if (variant < 0 || variant >= V_COUNT || !a0 || !b || !c || M <= 0 || N <= 0 || K0 <= 0 || K1 < 0 || iters <= 0 || (taps != 1 && taps != 9)) return NATINF_EINVAL;
    // the row-major epilogues store 8 columns at a time (only n < N is checked); 3x3: 64-channel chunks (the packed K order), whole
    // zero-bordered images, one batch index (a_bs would have to be the padded image size, and a1 shares it)
    if (K0 % taps || N % 8 || (a1 != nullptr) != (K1 > 0)) return NATINF_EINVAL;
    if (taps == 9 && ((K0 / 9) % BK || logW < 1 || logW > 12 || M % (1 << (2 * logW)) || batch != 1)) return NATINF_EINVAL;
    if (!variant_shipped(variant) || variant == V_CONV_GN || variant == V_FP8_256x256) return NATINF_ESTATE;      // retired variants; operand-type-specific kernels
#ifndef NATINF_DEV
    if (c_f32 >= 2) return NATINF_ESTATE;      // timing experiments: -DNATINF_DEV builds
#endif
    static bool configured = false;
    if (!configured) { if (!configure_gemm_kernels()) return NATINF_ENODEV; configured = true; }
    GemmArgs g = gemm_defaults();
    g.a0 = (const bf16*)a0; g.a0_C = K0 / taps; g.a0_ld = g.a0_C; g.taps = taps; g.logW = logW; g.logHW = 2 * logW; g.a0_padded = taps == 9;
    if (a1) { g.a1 = (const bf16*)a1; g.a1_C = K1; g.a1_ld = K1; }
    g.M = M; g.N = N; g.b = (const bf16*)b; g.b_ld = K0 + (a1 ? K1 : 0); g.batch = batch;
    if (batch > 1) { g.a_bs = (int64_t)M * g.a0_ld; g.b_bs = (int64_t)N * g.b_ld; g.c_bs = (int64_t)M * N; }
    g.bias_n = bias_n; g.scale = scale; g.c = c; g.c_ld = N; g.c_mode = c_f32 == 1 ? OUT_F32 : (c_f32 >= 2 ? 100 + c_f32 : OUT_BF16);      // >= 2: timing experiments (tools/bench_gemm.py)
    g.dbg_ts = g_dbg_ts;
    g.splitk_ws = g_dbg_splitk_ws; g.splitk_max = g_dbg_splitk_max;
    const int saved = g_force_variant;
    g_force_variant = variant;
    g_launch_error = 0;
    for (int i = 0; i < iters; ++i) launch_gemm(g, (hipStream_t)stream);
    g_force_variant = saved;
    if (g_launch_error) { g_launch_error = 0; return NATINF_EINVAL; }
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

// natinf_debug_set_conv_operand: the next natinf_debug_gemm_fused call is a 3x3 implicit convolution (taps == 9) -- see include/natinf_ncsnpp.h
int g_dbg_conv_logW = 0; const void* g_dbg_conv_a1 = nullptr; int g_dbg_conv_c1 = 0;
int natinf_debug_set_conv_operand(int logW, const void* a1, int c1) {
    if (logW < 0 || logW > 12 || c1 < 0 || c1 % BK || (c1 > 0) != (a1 != nullptr) || (logW == 0 && a1)) return NATINF_EINVAL;
    g_dbg_conv_logW = logW; g_dbg_conv_a1 = a1; g_dbg_conv_c1 = c1;
    return NATINF_OK;
}

// One plain GEMM C = A B^T with the fused epilogue terms of GemmArgs (tests/test_gpu_gemm_epilogue.py): every pointer but a / b / c
// may be NULL.  rowvec / gate are [samples][N] tables indexed by row >> log_rows_per_sample; gn_part receives (sum, sum of
// squares) per block tile and 4-column quad ([ceil(M / *bm_out)][N / 4] float2).  fp32_slab forces the general epilogue.
int natinf_debug_gemm_fused(int variant, int M, int N, int K, const void* a, const void* b, const float* bias_n, const float* bias_m,
                            const float* rowvec, const float* gate, int log_rows_per_sample, const void* resid_bf16, const float* resid_f32,
                            float scale, int act, void* c, int c_f32, float* gn_part, int* bm_out, int fp32_slab, natinf_stream_t stream) {
    const int logW = g_dbg_conv_logW, c1 = g_dbg_conv_c1;              // natinf_debug_set_conv_operand: consumed by this call, whatever its outcome
    const void* a1 = g_dbg_conv_a1;
    g_dbg_conv_logW = 0; g_dbg_conv_a1 = nullptr; g_dbg_conv_c1 = 0;
    if (variant < 0 || variant >= V_COUNT || !a || !b || !c || M <= 0 || N <= 0 || K <= 0 || c_f32 < 0 || c_f32 > 2) return NATINF_EINVAL;
    if (c_f32 == 2) {                          // NCHW fp32 (the VAE's output head): bias and scale only, whole images
        if (!logW || bias_m || rowvec || gate || resid_bf16 || resid_f32 || gn_part || act != ACT_NONE) return NATINF_EINVAL;
    } else if (N % 8) return NATINF_EINVAL;
    if (logW && (K % 9 || (K / 9) % BK || M % (1 << (2 * logW)))) return NATINF_EINVAL;
    if (!variant_shipped(variant) || variant == V_CONV_GN || variant == V_FP8_256x256) return NATINF_ESTATE;
    if (!configure_gemm_kernels()) return NATINF_ENODEV;
    GemmArgs g = gemm_defaults();
    g.a0 = (const bf16*)a; g.a0_C = K; g.a0_ld = K; g.M = M; g.N = N; g.b = (const bf16*)b; g.b_ld = K;
    if (logW) {
        g.taps = 9; g.a0_C = g.a0_ld = K / 9; g.logW = logW; g.logHW = 2 * logW; g.a0_padded = 1; g.b_ld = K + c1;
        if (a1) { g.a1 = (const bf16*)a1; g.a1_C = g.a1_ld = c1; }
    }
    g.bias_n = bias_n; g.bias_m = bias_m; g.rowvec = rowvec; g.rowvec_ld = N; g.gate = gate; g.gate_ld = N; g.log_rows_per_sample = log_rows_per_sample;
    g.resid = (const bf16*)resid_bf16; g.resid_ld = N; g.resid_f32 = resid_f32; g.resid_f32_ld = N;
    g.scale = scale; g.act = act; g.c = c; g.c_ld = N; g.c_mode = c_f32 == 2 ? OUT_F32_NCHW : (c_f32 ? OUT_F32 : OUT_BF16);
    g.gn_part = gn_part; g.gn_quads = N / 4; g.epi_fp32_slab = fp32_slab != 0;
    g.splitk_ws = g_dbg_splitk_ws; g.splitk_max = g_dbg_splitk_max;
    g.dbg_ts = g_dbg_ts;
    const int saved = g_force_variant;
    g_force_variant = variant;
    g_launch_error = 0;
    const int bm = launch_gemm(g, (hipStream_t)stream);
    g_force_variant = saved;
    if (bm_out) *bm_out = bm;
    if (g_launch_error) { g_launch_error = 0; return NATINF_EINVAL; }
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

// The fused GroupNorm-apply + SiLU + 3x3 convolution kernel on its own (tests/test_gpu_conv_gn.py, tools/bench_conv_gn.py):
//   out[m, n] = (sum_{tap, c} silu(x[pixel(m) + tap, c] * scale[b, c] + shift[b, c]) * w[n, c, tap]  +  sum_c a1[m, c] * w1[n, c]
//                + bias[n] + resid[m, n]) * out_scale,   zero padding outside the image (applied AFTER the activation).
// x: raw bf16 [B][res][res][cin]; w_packed: bf16 [N][9*cin + c1] in the engine's K order ((c / 64) * 9 + tap) * 64 + c % 64, then
// the c1 shortcut columns; a1: bf16 [B*res*res][c1] or NULL (c1 = 0); resid: bf16 [M][N] or NULL; gn_part: NULL or
// [M / 256][N / 4] float2 partial (sum, sum of squares) of the outputs.  The kernel takes its operands in FOLDED form
// (GemmArgs::gn_folded): the caller passes scale * -log2(e), shift * -log2(e) and the 3x3 columns of w_packed * -ln 2.
int g_dbg_cg_up = 0;
// bit 0: the next natinf_debug_conv_gn calls read x as [B][res/2][res/2][cin] through the kernel's nearest-2x up-sampling fetch (GemmArgs::a0_up);
// bit 1: the same for a1 ([B*(res/2)^2][c1], GemmArgs::a1_up) -- the fetch paths of the up-sampling res-blocks (natinf_set_fuse_up)
int natinf_debug_conv_gn_up(int flags) { if (flags & ~3) return NATINF_EINVAL; g_dbg_cg_up = flags; return NATINF_OK; }
// the consumer's GroupNorm table from the producing tile (GemmArgs::fin_*; tests/test_gpu_gn_partials.py): the following natinf_debug_conv_gn calls pass these on -- the tiles
// that hold whole samples x every channel (N = 256: k_conv_gn3 at 16x16, k_conv_gn2 at 8x8 / 4x4) then write fin_scale / fin_shift [B][N].  fin_scale = NULL: off again.
float* g_dbg_fin_scale = nullptr; float* g_dbg_fin_shift = nullptr; const float* g_dbg_fin_gamma = nullptr; const float* g_dbg_fin_beta = nullptr;
int g_dbg_fin_cg = 0; float g_dbg_fin_mul = 1.0f;
int natinf_debug_conv_gn_fin(float* fin_scale, float* fin_shift, const float* gamma, const float* beta, int channels_per_group, float mul) {
    if (fin_scale && (!fin_shift || !gamma || !beta || channels_per_group < 4 || channels_per_group % 4)) return NATINF_EINVAL;
    g_dbg_fin_scale = fin_scale; g_dbg_fin_shift = fin_shift; g_dbg_fin_gamma = gamma; g_dbg_fin_beta = beta; g_dbg_fin_cg = channels_per_group; g_dbg_fin_mul = mul;
    return NATINF_OK;
}
int natinf_debug_conv_gn(int res, int B, int N, int cin, int c1, const void* x, const float* scale, const float* shift, const void* w_packed,
                         void* w_frag, const void* a1, const float* bias_n, const void* resid, float out_scale, void* out, float* gn_part, int iters,
                         natinf_stream_t stream) {
    if ((res != 32 && res != 16 && res != 8 && res != 4) || B <= 0 || N <= 0 || N % 8 || cin <= 0 || cin % 64 || c1 < 0 || c1 % 64 || (c1 > 0) != (a1 != nullptr) ||
        !x || !scale || !shift || !w_packed || !out || iters <= 0) return NATINF_EINVAL;
    static bool configured = false;
    if (!configured) { if (!configure_gemm_kernels()) return NATINF_ENODEV; configured = true; }
    GemmArgs g = gemm_defaults();
    g.a0 = (const bf16*)x; g.a0_ld = cin; g.a0_C = cin; g.taps = 9; g.logW = ilog2(res); g.logHW = 2 * g.logW;
    g.gn_scale = scale; g.gn_shift = shift; g.gn_ld = cin; g.gn_folded = 1;
    if (a1) { g.a1 = (const bf16*)a1; g.a1_ld = c1; g.a1_C = c1; }
    g.M = B * res * res; g.N = N; g.b = (const bf16*)w_packed; g.b_ld = 9 * cin + c1; g.bias_n = bias_n;
    g.resid = (const bf16*)resid; g.resid_ld = N; g.scale = out_scale; g.c = out; g.c_ld = N;
    g.gn_part = gn_part; g.gn_quads = N / 4;
    if (g_dbg_fin_scale) {                                           // natinf_debug_conv_gn_fin
        if (!gn_part || N != 256 || res > 16 || N % g_dbg_fin_cg) return NATINF_EINVAL;
        g.fin_scale = g_dbg_fin_scale; g.fin_shift = g_dbg_fin_shift; g.fin_gamma = g_dbg_fin_gamma; g.fin_beta = g_dbg_fin_beta;
        g.fin_ld = N; g.fin_cg = g_dbg_fin_cg; g.fin_mul = g_dbg_fin_mul; g.fin_eps = GN_EPS;
    }
    g.dbg_ts = g_dbg_ts;
    g.a0_up = g_dbg_cg_up & 1; g.a1_up = (a1 && (g_dbg_cg_up & 2)) ? 1 : 0;      // natinf_debug_conv_gn_up: x / a1 are given at HALF the resolution
    if (w_frag && N % 16 == 0) g.b_frag = (const bf16*)w_frag;      // k_conv_gn2 (used when N is a whole number of its column tiles): w_frag receives the fragment-major copy
    if (!conv_gn_ok(g)) return NATINF_EINVAL;                        // (shipped builds: k_conv_gn2 only -- w_frag is required and N % 128 == 0)
    if (g.b_frag) {
        const int64_t n = (int64_t)(N / 16) * (9 * (cin / 32) + c1 / 32) * 64;
        hipLaunchKernelGGL(k_pack_frag, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, (hipStream_t)stream, (const bf16*)w_packed, (bf16*)w_frag, N, g.b_ld, cin, c1);
    }
    for (int i = 0; i < iters; ++i) launch_gemm(g, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

// k_fold_up_conv on its own (tests/test_gpu_up_fold.py): w [N][cin][3][3] fp32 -> out_f32 (may be NULL) [2][2][N][cin][2][2], the folded phase kernels times w_mul before the
// bf16 rounding, and out_packed (may be NULL) bf16 [4 N][4 cin], what the up-fold launch multiplies with
int natinf_debug_fold_up_weights(const float* w, int N, int cin, float w_mul, float* out_f32, void* out_packed, natinf_stream_t stream) {
    if (!w || N <= 0 || cin <= 0 || (!out_f32 && !out_packed) || (out_packed && cin % 64)) return NATINF_EINVAL;
    ncsn_upf::fold(w, out_packed, out_f32, N, cin, w_mul, stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
// Conv_0 of the 16 -> 32 up-sampling block as the plan with natinf_set_fuse_up_fold(1) runs it (tests/test_gpu_up_fold.py): k_fold_up_conv, k_gn_apply at 16x16, the up-fold launch.
//   out[pixel (2 i + a, 2 j + b) of sample s, n] = (sum_{ty, tx, c} silu(x[s, i + a - 1 + ty, j + b - 1 + tx, c] * scale[s, c] + shift[s, c]) * Wp[a][b][n, c, ty, tx] + bias[n] + rowvec[s, n]) * out_scale
//   = conv3x3(nearest_up_2x(silu(x * scale + shift)), w, zero padding) + ...   x: raw bf16 [B][16][16][cin]; scale / shift [B][cin] PLAIN (this form does not fold -log2 e into
// them); w: fp32 [N][cin][3][3], N = 256; w_packed: scratch, bf16 [4 N][4 cin]; h_scratch: bf16 [B][18][18][cin]; rowvec: NULL or [B][N]; out: bf16 [B * 1024][N];
// gn_part: NULL or [4 B][N / 4] float2 -- row 4 s + 2 a + b = the (sum, sum of squares) of sample s's outputs of parity (a, b).
int natinf_debug_conv_up_fold(int B, int N, int cin, const void* x, const float* scale, const float* shift, const float* w, void* w_packed, void* h_scratch,
                              const float* bias_n, const float* rowvec, float out_scale, void* out, float* gn_part, int iters, natinf_stream_t stream) {
    if (B <= 0 || N != UPFOLD_BN || cin <= 0 || cin % 64 || !x || !scale || !shift || !w || !w_packed || !h_scratch || !out || iters <= 0) return NATINF_EINVAL;
    static bool configured = false;
    if (!configured) { if (!configure_gemm_kernels()) return NATINF_ENODEV; configured = true; }
    hipStream_t s = (hipStream_t)stream;
    constexpr int W = UPFOLD_W, logW = 4;
    ncsn_upf::fold(w, w_packed, nullptr, N, cin, 1.0f, stream);
    hipLaunchKernelGGL(k_gn_apply, dim3((unsigned)((W + 2 + GN_ROWS - 1) / GN_ROWS), (unsigned)B), dim3(256), 0, s, (const bf16*)x, cin, cin, logW, 2 * logW, scale, shift,
                       (bf16*)h_scratch, (bf16*)nullptr, ACT_SILU, RS_NONE, 1);
    GemmArgs g = gemm_defaults();
    g.a0 = (const bf16*)h_scratch; g.a0_ld = cin; g.a0_padded = 1; g.a0_C = cin; g.taps = 4; g.logW = logW; g.logHW = 2 * logW;
    g.M = B * W * W; g.N = 4 * N; g.b = (const bf16*)w_packed; g.b_ld = 4 * cin; g.bias_n = bias_n;
    g.rowvec = rowvec; g.rowvec_ld = N; g.log_rows_per_sample = 2 * logW; g.scale = out_scale;
    g.c = out; g.c_ld = N; g.gn_part = gn_part; g.gn_quads = N / 4;
    if (!up_fold_epi(g)) return NATINF_EINVAL;
    g_launch_error = 0;
    for (int i = 0; i < iters; ++i) launch_gemm(g, s);
    if (g_launch_error) { g_launch_error = 0; return NATINF_EINVAL; }
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

// One 16x16 attention block on caller-supplied operands (tests/test_gpu_attn_block_alone.py): the engine's own packs and launches (pack_attn_* / launch_attn_*
// above), nothing else.  bias [4][256]: rows 0, 1 ARE the engine's bqk table (q then k), rows 2, 3 its bv and b3.
int natinf_debug_attn_block(int plan, int B, const void* x, int x_ld, const float* scale, const float* shift, const float* w, const float* bias,
                            void* packed, void* scratch, void* out, int o_ld, float out_scale, float* gn_part, natinf_stream_t stream) {
    if (plan < 0 || plan > 2 || B < 1 || !x || !scale || !shift || !w || !bias || !packed || !out || x_ld < 256 || x_ld % 8 || o_ld < 256 || o_ld % 8 ||
        (plan != 2 && !scratch)) return NATINF_EINVAL;
    static bool configured = false;
    if (!configured) { if (!configure_gemm_kernels()) return NATINF_ENODEV; configured = true; }
    constexpr int64_t WW = 256 * 256;
    unsigned char* pk = reinterpret_cast<unsigned char*>(packed);
    hipStream_t s = (hipStream_t)stream;
    AttnBlk256 a;
    a.plan = plan; a.B = B; a.x = (const bf16*)x; a.x_ld = x_ld; a.sc = scale; a.sh = shift;
    a.out = (bf16*)out; a.o_ld = o_ld; a.out_scale = out_scale; a.gn_part = reinterpret_cast<float2*>(gn_part); a.gn_quads = 64;
    if (plan == 2) {
        float* fq = reinterpret_cast<float*>(pk + NATINF_ATTN_BLOCK_OFF_FOLD_WQK); float* fv = reinterpret_cast<float*>(pk + NATINF_ATTN_BLOCK_OFF_FOLD_WVO);
        float* cq = reinterpret_cast<float*>(pk + NATINF_ATTN_BLOCK_OFF_FOLD_CQ); float* bo = reinterpret_cast<float*>(pk + NATINF_ATTN_BLOCK_OFF_FOLD_BO);
        bf16* wqf2 = reinterpret_cast<bf16*>(pk + NATINF_ATTN_BLOCK_OFF_WQK_PACKED); bf16* wvof2 = reinterpret_cast<bf16*>(pk + NATINF_ATTN_BLOCK_OFF_WVO_PACKED);
        pack_attn_fold(w, w + WW, w + 2 * WW, w + 3 * WW, bias, bias + 512, bias + 768, fq, cq, fv, bo, wqf2, wvof2, s);
        a.wqf2 = wqf2; a.cq2 = cq; a.wvof2 = wvof2; a.bo2 = bo;
    } else {
        bf16* wqkvf = reinterpret_cast<bf16*>(pk + NATINF_ATTN_BLOCK_OFF_WQKV); bf16* w3f = reinterpret_cast<bf16*>(pk + NATINF_ATTN_BLOCK_OFF_W3);
        pack_attn_qkv_w(w, w + WW, w + 2 * WW, wqkvf, s);
        pack_attn_w3(w + 3 * WW, w3f, s);
        a.wqkvf = wqkvf; a.bqk = bias; a.bv = bias + 512; a.w3f = w3f; a.b3 = bias + 768;
        a.qk = reinterpret_cast<bf16*>(scratch); a.vT = a.qk + (int64_t)B * 256 * 512;
        if (plan == 0) launch_attn_qkv256(a, s);
    }
    launch_attn_blk256(a, s);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_debug_quant_fp8_rows(const float* w, void* q, float* row_scale, int rows, int cols, natinf_stream_t stream) {
    if (!w || !q || !row_scale || rows <= 0 || cols <= 0 || cols % 2) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_pack_fp8_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, w, (uint8_t*)q, row_scale, rows, cols);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_debug_gemm_fp8(int M, int N, int K, const void* a8, const float* a_scale, const void* a_mx, const void* b8, const float* b_scale,
                          const float* bias_n, void* c, void* c_mx, int c_mode, int iters, natinf_stream_t stream) {
    if (!a8 || !b8 || !c || M <= 0 || N <= 0 || K <= 0 || K % 128 || N % 8 || iters <= 0) return NATINF_EINVAL;
    static bool configured = false;
    if (!configured) { if (!configure_gemm_kernels()) return NATINF_ENODEV; configured = true; }
    GemmArgs g = gemm_defaults();
    g.a0 = (const bf16*)a8; g.a0_C = K; g.a0_ld = K; g.M = M; g.N = N; g.b = (const bf16*)b8; g.b_ld = K;
    const int act = c_mode >> 8; c_mode &= 0xff;                         // bits 8+: activation (2 = tanh-GELU: with c_mode 3 the fc1 epilogue of the MMDiT engine)
    if (act != ACT_NONE && act != ACT_GELU_TANH) return NATINF_EINVAL;
    g.deq_m = a_scale; g.deq_n = b_scale; g.bias_n = bias_n; g.c = c; g.c_ld = N; g.c_mode = c_mode; g.act = act;
    g.a_mx = (const uint8_t*)a_mx; g.a_mx_ld = M; g.c_mx = (uint8_t*)c_mx; g.c_mx_ld = M;       // K-tile-major planes of M rows
    if ((c_mode == OUT_FP8_MX && (!c_mx || N % 32)) || c_mode < 0 || c_mode > OUT_FP8_MX || c_mode == OUT_F32_NCHW) return NATINF_EINVAL;
    for (int i = 0; i < iters; ++i) launch_gemm_fp8(g, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

// timing experiments: device buffer of 16 uint64 s_memtime stamps written by block 0 / thread 0 of natinf_debug_gemm launches
int natinf_debug_timestamps(void* dev_buf16) {
#ifdef NATINF_DEV
    g_dbg_ts = reinterpret_cast<unsigned long long*>(dev_buf16); return NATINF_OK;
#else
    (void)dev_buf16; return NATINF_ESTATE;             // the shipped kernels carry no stamps (make EXTRA=-DNATINF_DEV)
#endif
}

int natinf_set_gemm_raster(int rows) { g_raster_g = rows; return NATINF_OK; }
int natinf_set_fuse_gn(int on) { g_fuse_gn = on != 0; return NATINF_OK; }
int natinf_set_fuse_gn8(int on) { g_fuse_gn8 = on != 0; return NATINF_OK; }
int natinf_set_attn256(int on) { return on ? NATINF_OK : NATINF_ESTATE; }      // (0: k_attn_fused<8,16,true>, retired)
int natinf_set_conv_gn_warm(int mask) { if (mask < 0 || mask > 15) return NATINF_EINVAL; g_cg_warm = mask; return NATINF_OK; }
int natinf_set_attn_block(int on) { g_attn_blk = on < 0 ? ATTN_BLK_DEFAULT : (on > 2 ? 2 : on); return NATINF_OK; }
int natinf_set_attn_qkv(int on) { g_attn_qkv = on != 0; return NATINF_OK; }
int natinf_set_attn_waves8(int on) { g_attn_w8 = on != 0; return NATINF_OK; }
int natinf_set_attn_proj(int on) { g_attn_proj = on != 0; return NATINF_OK; }
int natinf_set_fuse_fin(int on) {              // 1 = every level that can (the default), 0 = none, 2 = 8x8 / 4x4 only (the round-4 plan), 3 = 16x16 only
    if (on < 0 || on > 3) return NATINF_EINVAL;
    static const int mask[4] = {0, 3, 1, 2};    // g_fuse_fin: bit 0 = 8x8 / 4x4 (k_conv_gn2), bit 1 = 16x16 (k_conv_gn3)
    g_fuse_fin = mask[on];
    return NATINF_OK;
}
int natinf_set_gemm_round_model(int on) { g_round_model = on != 0; g_round_model_w128 = on >= 10 ? on : 13; return NATINF_OK; }
int natinf_set_gemm_w128(int on) { g_w128 = on < 0 ? 0 : (on > 2 ? 2 : on); return NATINF_OK; }
int natinf_set_fuse_gn4(int on) { g_fuse_gn4 = on != 0; return NATINF_OK; }
int natinf_set_conv_gn8_tile(int one_image) { return one_image ? NATINF_OK : NATINF_ESTATE; }      // (0: the two-image tile, retired)
int natinf_set_fuse_head(int on) { g_fuse_head = on != 0; return NATINF_OK; }
int natinf_set_conv_gn_w128(int mask) { if (mask < 0 || mask > 7) return NATINF_EINVAL; g_cg3 = mask; return NATINF_OK; }
int natinf_set_conv_gn_w128_min_k(int shape, int k) { if (shape < 0 || shape > 2 || k < 0) return NATINF_EINVAL; g_cg3_min_k[shape] = k; return NATINF_OK; }
int natinf_set_conv_gn_wide(int mask) { if (mask < 0 || mask > 3) return NATINF_EINVAL; g_cg_wide = mask; return NATINF_OK; }
int natinf_set_conv_gn_regw(int on) { return on ? NATINF_OK : NATINF_ESTATE; }      // (0: k_conv_gn, the LDS-ring form, retired)
int natinf_set_fuse_up(int on) { g_fuse_up = on != 0; return NATINF_OK; }
int natinf_set_fuse_up_fold(int on) { g_fuse_up_fold = on < 0 ? UP_FOLD_DEFAULT : on != 0; return NATINF_OK; }      // (negative: the library's default)
int natinf_set_gemm_splitk(int on) { g_splitk = on != 0; return NATINF_OK; }
int natinf_debug_set_splitk_workspace(float* ws, int max_slices) { g_dbg_splitk_ws = ws; g_dbg_splitk_max = ws ? max_slices : 0; return NATINF_OK; }
int natinf_set_gemm_half_issue(int on) { return on ? NATINF_OK : NATINF_ESTATE; }      // (0: the every-wave-issues pipelines, retired)
int natinf_set_gemm_pref512(int on) { g_pref_512 = on != 0; return NATINF_OK; }
int natinf_set_gemm_epilogue(int fp32_slab) { g_epi_fp32_slab = fp32_slab != 0; return NATINF_OK; }

int natinf_set_gemm_variant(int variant) {
    if (variant < 0 || variant >= V_COUNT) return NATINF_EINVAL;
    if (!variant_shipped(variant) || variant == V_CONV_GN || variant == V_FP8_256x256) return NATINF_ESTATE;      // retired variants; operand-type-specific kernels
    g_force_variant = variant;
    return NATINF_OK;
}

int natinf_gemm_profile(int enable) { g_gemm_prof.on = enable != 0; return NATINF_OK; }
int natinf_gemm_profile_read(char* buf, int cap) {
    if (!buf || cap <= 0) return NATINF_EINVAL;
    std::map<std::string, std::pair<double, int64_t>> by;
    std::vector<std::string> order;
    int rc = NATINF_OK;
    for (auto& e : g_gemm_prof.ev) {
        float ms = 0.f;
        if (hipEventSynchronize(e.b) != hipSuccess || hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) { (void)hipGetLastError(); rc = NATINF_ELAUNCH; }
        else {
            auto it = by.find(e.tag);
            if (it == by.end()) { order.push_back(e.tag); it = by.emplace(e.tag, std::make_pair(0.0, (int64_t)0)).first; }
            it->second.first += ms; it->second.second += 1;
        }
        g_gemm_prof.pool.emplace_back(e.a, e.b);
    }
    g_gemm_prof.ev.clear();
    if (rc != NATINF_OK) return rc;
    std::string out;
    for (auto& t : order) {
        char tail[64];
        snprintf(tail, sizeof(tail), " %lld %.6f\n", (long long)by[t].second, by[t].first);
        out += t + tail;
    }
    if ((int)out.size() + 1 > cap) return NATINF_EINVAL;
    memcpy(buf, out.c_str(), out.size() + 1);
    return (int)out.size();
}
int natinf_ncsnpp_profile(natinf_ncsnpp_t h, int enable) {
    if (!h) return NATINF_EINVAL;
    h->prof = enable != 0;
    return NATINF_OK;
}

int natinf_ncsnpp_profile_read(natinf_ncsnpp_t h, double* ms_by_class, int64_t* launches_by_class) {
    if (!h || !ms_by_class || !launches_by_class) return NATINF_EINVAL;
    for (int i = 0; i < N_CLS; ++i) { ms_by_class[i] = 0.0; launches_by_class[i] = 0; }
    for (const auto& r : h->recs) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) {
            (void)hipGetLastError();
            return NATINF_ELAUNCH;
        }
        ms_by_class[r.cls] += ms; launches_by_class[r.cls] += 1;
        h->pool.push_back(r.a); h->pool.push_back(r.b);
    }
    h->recs.clear();
    return NATINF_OK;
}

int natinf_ncsnpp_debug_tap(natinf_ncsnpp_t h, int module_idx, float* out, int64_t capacity_elems, natinf_stream_t stream) {
    if (!h || !out) return NATINF_EINVAL;
    if (!(h->flags & NATINF_NCSNPP_KEEP_ACTIVATIONS) || !h->last_ws) return NATINF_ESTATE;
    auto it = h->taps.find(module_idx);
    if (it == h->taps.end()) return NATINF_EINVAL;
    const TRef& t = it->second;
    const int HW = t.res * t.res;
    const int64_t total = (int64_t)h->last_B * t.C * HW;
    if (capacity_elems < total) return NATINF_EINVAL;
    const bf16* src = reinterpret_cast<const bf16*>(h->last_ws + t.off * h->last_B) + t.coff;
    hipLaunchKernelGGL(k_nhwc_to_nchw_f32, dim3(grid1d(total, 256, 1 << 30)), dim3(256), 0, (hipStream_t)stream, src, t.ld, t.C, HW, out, total);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

// The GroupNorm, output-head and glue kernels alone (include/natinf_ncsnpp.h; tests/test_gpu_gn_kernels.py): the grid and block expressions of emit_gn_stats,
// emit_gn_from_parts, emit_gn_apply, the head op and the embedding / stem / pack / tap launches above.  Every precondition a kernel leaves to its caller is
// NATINF_EINVAL here, before anything is launched; no plan of the library launches outside them (kernel table: k_time_embed's capped grid was the exception).
static bool dbg_misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

int natinf_debug_gn_stats(const void* x, int ld, int C, int HW, int B, const float* gamma, const float* beta, float* scale, float* shift, float eps, float out_mul,
                          natinf_stream_t stream) {
    if (!x || !gamma || !beta || !scale || !shift || B < 1 || HW < 1 || C < 32 || C > 512 || C % 32 || ld < C || ld % 8 || dbg_misaligned(x, 16)) return NATINF_EINVAL;
    if ((256 / (C >> 3)) * C > 16 * 128 + 64) return NATINF_EINVAL;      // s_part (never true for C % 8 == 0: lanes * C <= 2048; kept next to the array it guards)
    hipLaunchKernelGGL(k_gn_stats, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ld, C, HW, gamma, beta, scale, shift, eps, out_mul);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_debug_gn_finalize(const float* P0, int tps0, int quads0, const float* P1, int tps1, int quads1, int C, int HW, int B, const float* gamma, const float* beta,
                             float* scale, float* shift, float eps, float out_mul, natinf_stream_t stream) {
    if (!P0 || !gamma || !beta || !scale || !shift || B < 1 || HW < 1 || tps0 < 1 || quads0 < 1) return NATINF_EINVAL;
    if (P1 ? (tps1 < 1 || quads1 < 1) : (tps1 != 0 || quads1 != 0)) return NATINF_EINVAL;
    // C % 128: qpg = (C / 32) >> 2 quads per group (0 below 128: the table would be gamma / sqrt(eps)); s_p[128]; every quad of the C channels is summed
    if (C < 128 || C > 512 || C % 128 || quads0 + quads1 > 128 || (quads0 + quads1) * 4 != C || dbg_misaligned(P0, 8) || dbg_misaligned(P1, 8)) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_gn_finalize, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(P0), tps0, quads0,
                       reinterpret_cast<const float2*>(P1), tps1, quads1, C, HW, gamma, beta, scale, shift, eps, out_mul);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_debug_gn_apply(const void* x, int ld, int C, int logW, int logHW, int B, const float* scale, const float* shift, void* y, void* xr, int act, int mode, int pad,
                          natinf_stream_t stream) {
    if (!x || !scale || !shift || !y || B < 1 || B > 65535 || C < 8 || C % 8 || (C >> 3) > 256 || ld < C || ld % 8) return NATINF_EINVAL;
    if (logW < 0 || logHW < logW || logHW > 24 || mode < RS_NONE || mode > RS_DOWN || (pad != 0 && pad != 1) || (act != ACT_NONE && act != ACT_SILU)) return NATINF_EINVAL;
    if (mode == RS_DOWN && (logW < 1 || logHW - logW < 1)) return NATINF_EINVAL;
    if (dbg_misaligned(x, 16) || dbg_misaligned(y, 16) || dbg_misaligned(xr, 16) || dbg_misaligned(scale, 16) || dbg_misaligned(shift, 16)) return NATINF_EINVAL;
    const int Hs = 1 << (logHW - logW), Hd = mode == RS_UP ? 2 * Hs : (mode == RS_DOWN ? Hs / 2 : Hs);
    const int rows_per_img = Hd + 2 * pad;
    hipLaunchKernelGGL(k_gn_apply, dim3((unsigned)((rows_per_img + GN_ROWS - 1) / GN_ROWS), (unsigned)B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ld, C,
                       logW, logHW, scale, shift, (bf16*)y, (bf16*)xr, act, mode, pad);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_debug_head_conv(const void* x, int ld, int B, const float* scale, const float* shift, const void* w16, const float* bias, float* out, natinf_stream_t stream) {
    if (!x || !scale || !shift || !w16 || !bias || !out || B < 1 || ld < HeadConvCfg::C || ld % 8) return NATINF_EINVAL;
    if (dbg_misaligned(x, 16) || dbg_misaligned(w16, 16) || dbg_misaligned(out, 16)) return NATINF_EINVAL;
    // the engine's init (configure_ncsnpp_kernels): 49,472 bytes of dynamic LDS need the attribute
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_head_conv), hipFuncAttributeMaxDynamicSharedMemorySize, HeadConvCfg::LDS_BYTES) != hipSuccess) {
        (void)hipGetLastError();
        return NATINF_ENODEV;
    }
    hipLaunchKernelGGL(k_head_conv, dim3((unsigned)(B * (HeadConvCfg::RES / HeadConvCfg::ROWS))), dim3(256), HeadConvCfg::LDS_BYTES, (hipStream_t)stream,
                       (const bf16*)x, ld, scale, shift, (const bf16*)w16, bias, out);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_debug_time_embed(const float* labels, void* emb, int B, natinf_stream_t stream) {
    if (!labels || !emb || B < 1 || B >= (1 << 21)) return NATINF_EINVAL;      // natinf_ncsnpp_forward's own limit (B * 1024 < 2^31); the index is an int
    hipLaunchKernelGGL(k_time_embed, dim3(grid1d((int64_t)B * 128, 256, 1 << 30)), dim3(256), 0, (hipStream_t)stream, labels, (bf16*)emb, B);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_debug_stem_im2col(const float* x, void* A, int B, natinf_stream_t stream) {
    if (!x || !A || B < 1 || B > (1 << 17) || dbg_misaligned(A, 16)) return NATINF_EINVAL;
    const int64_t rows = (int64_t)B * 1024;
    hipLaunchKernelGGL(k_stem_im2col, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (bf16*)A, rows);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_debug_pack_conv(const float* src, void* dst, int N, int Cin, int taps, int dst_ld, int koff, int tap_stride_c, int chunked, float wmul, natinf_stream_t stream) {
    if (!src || !dst || N < 1 || Cin < 1 || taps < 1 || koff < 0 || (chunked != 0 && chunked != 1)) return NATINF_EINVAL;
    const int64_t n = (int64_t)N * Cin * taps;
    // the last column a row of the source reaches must lie inside the destination row
    const int64_t span = chunked ? (int64_t)((Cin + 63) / 64) * taps * 64 : (int64_t)(taps - 1) * tap_stride_c + Cin;
    if ((!chunked && tap_stride_c < Cin) || koff + span > dst_ld || n > ((int64_t)1 << 30) * 256) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_pack_conv, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, (hipStream_t)stream, src, (bf16*)dst, N, Cin, taps, dst_ld, koff, tap_stride_c, chunked, wmul);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_debug_pack_transpose(const float* src, void* dst, int K, int N, int dst_ld, natinf_stream_t stream) {
    if (!src || !dst || K < 1 || N < 1 || dst_ld < K) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_pack_transpose, dim3(grid1d((int64_t)K * N, 256, 1 << 30)), dim3(256), 0, (hipStream_t)stream, src, (bf16*)dst, K, N, dst_ld);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

int natinf_debug_nhwc_to_nchw(const void* x, int ld, int C, int HW, int B, float* out, natinf_stream_t stream) {
    if (!x || !out || B < 1 || C < 1 || HW < 1 || ld < C) return NATINF_EINVAL;
    const int64_t total = (int64_t)B * C * HW;
    if (total > ((int64_t)1 << 30) * 256) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_nhwc_to_nchw_f32, dim3(grid1d(total, 256, 1 << 30)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ld, C, HW, out, total);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

}  // extern "C"
#include "dit_engine.inc"
#include "mmdit_engine.inc"
#include "vae_engine.inc"
#include "inception_engine.inc"