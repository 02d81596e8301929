// gemm_launch.h -- the GEMM launch layer every engine calls: the tile variants and the choice among them (choose_variant), the epilogue a
// launch takes (packed_epi / fp8_epi), split-K, the fused-convolution shapes, launch_gemm / launch_gemm_fp8, and configure_gemm_kernels.
// Part of the one translation unit ncsnpp.hip.  Every shipped kernel instance is listed ONCE here -- a tile family (GemmFamilies), a fused
// convolution shape (ConvGnShapes), an fp8 family (Fp8Families) -- and configure / launch / the per-variant lookups all walk those lists:
// to add an instance, add it to its list.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "ncsnpp_kernels.h"
#include "gemm_dma.h"
#include "gemm_w128.h"
#include "conv_gn2.h"
#include "gemm_fp8.h"

using namespace ncsn;

// LDS sizes of the kernels an engine file owns: defined where the kernels are used
bool configure_conv_ring();                          // inception_engine.inc: the k_conv_ring instantiations
namespace { bool configure_ncsnpp_kernels();         // ncsnpp.hip: the output head and the 16x16 attention block
            bool configure_dit_attention();          // dit_engine.inc: the row-major-v forms of k_attn_fused
            bool configure_flash_attention(); }      // mmdit_engine.inc: the joint-sequence flash kernels
// k_conv_gn3 (conv_gn3.h / conv_gn3.hip: one wave per SIMD, 128 x 128 wave tiles, slot-table K loop) -- a translation unit of its own
// the guarded forms of the stream-writing kernels (stream_guard.hip, a translation unit of its own like conv_gn3.hip): the direct residual epilogue with GemmArgs::stream_guard on
// the five bf16 tile families that have it (EPI 10 beside 7) and on the four fp8 instances (EPI 4 beside 3), the split-K reduce and the patch embedding.  raster: g_raster_g
namespace ncsn_sg { bool configure(); bool has_tile(int variant); void launch_tile(const void* gemm_args, int variant, int raster, void* stream);
                    void launch_fp8(const void* gemm_args, int mxa, int w128, int raster, void* stream); void launch_splitk_reduce(const void* gemm_args, int slices, void* stream);
                    void launch_patch_embed(const float* z, const float* Wt, const float* bias, const float* pos, float* x, int C, int g, int D, int64_t rows, int x_f16, uint32_t* guard, void* stream); }
// the up-fold launch and its weight fold (up_fold.hip, a translation unit of its own as well): Conv_0 of the 16 -> 32 up-sampling block as four 2x2 phase convolutions
namespace ncsn_upf { bool configure(); void launch(const void* gemm_args, int epi, void* stream); void fold(const float* w, void* dst_bf16, float* dst_f32, int N, int Cin, float wmul, void* stream); }
namespace ncsn_cg3 { bool configure(); int tile_rows(int shape); int tile_cols(int shape); void launch(const void* gemm_args, int shape, int epi, void* stream); }

namespace {

// ------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------
int g_epi_fp32_slab = 0;           // natinf_set_gemm_epilogue(1): every launch takes the fp32-slab epilogue (A/B runs)
GemmArgs gemm_defaults() {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.epi_fp32_slab = g_epi_fp32_slab;
    g.taps = 1; g.batch = 1; g.scale = 1.0f; g.act = ACT_NONE; g.c_mode = OUT_BF16;
    return g;
}
// ------------------------------------------------------------------------------------------------
// GEMM kernel variants and the choice among them
// ------------------------------------------------------------------------------------------------
constexpr int NUM_CU = 256;
enum GemmVariant {
    V_AUTO = 0, V_GENERIC = 1,
    V_DMA_256x256 = 2, V_DMA_256x128 = 3, V_DMA_128x128 = 4,          // (retired: 2-stage, BK = 64)
    V_RING_256x256 = 5, V_RING_256x128 = 6, V_RING_128x128 = 7,       // (retired: NS-slot ring, BK = 32)
    V_RING_64x128 = 8,                                                 // NS-slot ring, BK = 32
    V_RING_256x128_W4 = 9,                                             // 4 waves, wave tile 128x64 (less LDS read traffic per MFMA)
    V_DMA_256x128_W4 = 10,                                             // (retired: the same tile, two-stage)
    V_DMA_256x256_S = 11, V_DMA_128x128_S = 12,                       // (retired: two-stage with the DMA issue spread between MFMA groups)
    V_DMA_512x128 = 13,                                                // (retired: 8 waves x (128x64), every wave issuing its own DMA)
    V_PATCH_256x256 = 14, V_PATCH_256x128 = 15,                        // (retired: 3x3 conv with an LDS-resident input patch)
    V_DMA_256x256_P = 16, V_DMA_256x128W4_P = 18,                      // (retired: two-stage + hand-counted LDS fragment pipeline)
    V_DMA_128x128_P = 17,                                              // two-stage + hand-counted LDS fragment pipeline
    V_8PH_256x256 = 19, V_8PH_NOPRIO = 20, V_8PH_READFIRST = 21, V_8PH_BOTH = 22,   // (retired: phase-interleaved schedule, counted vmcnt)
    V_FP8_256x256 = 23,                                                 // fp8 e4m3 operands (gemm_fp8.h); selected by GemmArgs::deq_m/deq_n callers only
    V_ABL_NODMA = 24, V_ABL_NOMFMA = 25,                                // (retired: K-loop ablations)
    V_DMA_256x256_H = 26, V_DMA_512x128_H = 27,                         // hand pipeline, DMA issued by one wave per SIMD only
    V_CONV_GN = 28,                                                     // 3x3 conv with fused GroupNorm-apply + SiLU of its input (conv_gn2.h); GemmArgs::gn_scale callers only
    V_W128 = 29,                                                        // 256x256x64, four waves with 128x128 wave tiles (one per SIMD, AGPR accumulators; gemm_w128.h)
    V_W128_A = 30, V_W128_D = 31, V_W128_X = 32,                        // (retired: other K-loop schedules of k_gemm_w128)
    V_COUNT
};
// Retired ids (superseded pipelines, tile shapes and ablations; their kernels are in git history before the commit that removed them): the numbering
// stays, natinf_set_gemm_variant / natinf_debug_gemm refuse them with NATINF_ESTATE.
const char* variant_name(int v) {
    static const char* n[] = {"auto", "generic128", "dma256x256", "dma256x128", "dma128x128", "ring256x256", "ring256x128",
                              "ring128x128", "ring64x128", "ring256x128w4", "dma256x128w4", "dma256x256s", "dma128x128s", "dma512x128", "patch256x256", "patch256x128", "dma256x256p", "dma128x128p", "dma256x128w4p", "gemm8ph", "gemm8ph_np", "gemm8ph_rf", "gemm8ph_nprf", "fp8_256x256", "abl_nodma", "abl_nomfma", "dma256x256h", "dma512x128h", "conv_gn", "w128_256x256", "w128_a", "w128_d", "w128_x"};
    return v >= 0 && v < V_COUNT ? n[v] : "?";
}
unsigned long long* g_dbg_ts = nullptr;
int g_force_variant = V_AUTO;
int g_round_model = 1;             // natinf_set_gemm_round_model(0): small-M plain GEMMs by the pre-round-4 rules (A/B runs)
int g_round_model_w128 = 13;       // cost of a round of k_gemm_w128 tiles in tenths of a round of 128 x 128 tiles (two blocks per CU)
int g_pref_512 = 1;                // N <= 128 layers with >= 2 tiles per CU: the 512x128 hand-pipelined tile (natinf_set_gemm_pref512: A/B runs)      // tuning / tests: force one variant for every DMA-eligible launch
std::string* g_record = nullptr;   // when set, launch_gemm describes the launch instead of issuing it

int g_raster_g = 8;                 // natinf_set_gemm_raster: row-tiles per raster group of wide-N launches (0 / 1 = plain row-major)
template <class Cfg, class K>
inline void launch_tiles(K kernel, const GemmArgs& g0, hipStream_t s) {
    const int nM = (g0.M + Cfg::BM_ - 1) / Cfg::BM_, nN = (g0.N + Cfg::BN_ - 1) / Cfg::BN_;
    GemmArgs g = g0;
    g.raster_g = (g_raster_g > 1 && nN >= 8 && nM >= g_raster_g) ? g_raster_g : 0;
    hipLaunchKernelGGL(kernel, dim3(nM * nN, 1, g.batch), dim3(Cfg::THREADS), Cfg::LDS_BYTES, s, g);
}
template <class Cfg, class K>
inline bool set_lds(K kernel) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES) == hipSuccess;
}
int g_cg_warm = 15;                // natinf_set_conv_gn_warm: bit mask by resolution (1: 4x4, 2: 8x8, 4: 16x16, 8: 32x32) of the fused-convolution launches that warm L2 with their weights

// Packed-epilogue specializations (EPI, gemm_dma.h) that exist per tile family, as bit masks: a launch whose epilogue is not
// instantiated for its tile takes the general fp32-slab epilogue (EPI 0: the same terms, the same single rounding).  Who needs what:
// 3 (SiLU) only the small time-embedding GEMMs; 4 (tanh-GELU), 7 (fp32 residual stream), 8 (row bias) the transformer engines, none
// of which ever reaches the N <= 128 tile.
constexpr unsigned EPI_ALL = 0x1FF;
template <unsigned MASK, int E, class F> inline void epi_case(F&& f) { if constexpr ((MASK >> E) & 1u) f(std::integral_constant<int, E>{}); }
template <unsigned MASK, class F> inline bool for_each_epi(F&& f) {             // f(integral_constant<int, E>) -> bool, over the instantiated ones; stops at the first false
    bool ok = true;
    auto one = [&](auto tag) { ok = ok && f(tag); };
    epi_case<MASK, 0>(one); epi_case<MASK, 1>(one); epi_case<MASK, 2>(one); epi_case<MASK, 3>(one); epi_case<MASK, 4>(one);
    epi_case<MASK, 5>(one); epi_case<MASK, 6>(one); epi_case<MASK, 7>(one); epi_case<MASK, 8>(one);
    return ok;
}
#define NATINF_EPI_OF(tag) decltype(tag)::value

// ---- the shipped kernel instances, each set listed once -----------------------------------------
// A family: the block-tile configuration (Cfg: BM_, BN_, THREADS, LDS_BYTES), the mask of epilogues it is instantiated for (EPI, bit 0 always
// set) and kernel<E>().  The instances of a family are exactly kernel<E>() for the E of its mask: configure_family sets their LDS sizes,
// launch_family runs the one a launch takes.
template <class... F> struct FamList {};
template <class Fam> bool configure_family() {
    return for_each_epi<Fam::EPI>([](auto t) { return set_lds<typename Fam::Cfg>(Fam::template kernel<NATINF_EPI_OF(t)>()); });
}
template <class... F> bool configure_families(FamList<F...>) { return (configure_family<F>() && ...); }
template <class Fam> void launch_family(int e, const GemmArgs& g, hipStream_t s) {      // e: an epilogue of Fam::EPI
    for_each_epi<Fam::EPI>([&](auto t) {
        if (NATINF_EPI_OF(t) != e) return true;
        launch_tiles<typename Fam::Cfg>(Fam::template kernel<NATINF_EPI_OF(t)>(), g, s);
        return false;
    });
}

// (1) the bf16 GEMM tile families, by variant id.  The library instantiates only the tile variants the dispatcher selects (choose_variant,
// splitk) plus the generic kernel; every other variant of the enum is retired
using CfgD256x256 = DmaCfg<2, 4, 8, 4>;
struct FamD128  { static constexpr int V = V_DMA_128x128_P;    using Cfg = DmaCfg<2, 2, 4, 4>;     static constexpr unsigned EPI = EPI_ALL;
                  template <int E> static constexpr auto kernel() { return &k_gemm_dma<2, 2, 4, 4, 2, E>; } };
struct FamRW4   { static constexpr int V = V_RING_256x128_W4;  using Cfg = RingCfg<2, 2, 8, 4, 3>; static constexpr unsigned EPI = EPI_ALL & ~(1u << 3);
                  template <int E> static constexpr auto kernel() { return &k_gemm_ring<2, 2, 8, 4, 3, E>; } };
struct FamR64   { static constexpr int V = V_RING_64x128;      using Cfg = RingCfg<2, 2, 2, 4, 4>; static constexpr unsigned EPI = EPI_ALL;
                  template <int E> static constexpr auto kernel() { return &k_gemm_ring<2, 2, 2, 4, 4, E>; } };
struct FamD256H { static constexpr int V = V_DMA_256x256_H;    using Cfg = CfgD256x256;            static constexpr unsigned EPI = EPI_ALL & ~(1u << 3);
                  template <int E> static constexpr auto kernel() { return &k_gemm_dma<2, 4, 8, 4, 6, E>; } };
struct FamD512H { static constexpr int V = V_DMA_512x128_H;    using Cfg = DmaCfg<4, 2, 8, 4>;     static constexpr unsigned EPI = EPI_ALL & ~((1u << 3) | (1u << 4) | (1u << 7) | (1u << 8));
                  template <int E> static constexpr auto kernel() { return &k_gemm_dma<4, 2, 8, 4, 6, E>; } };
struct FamW128  { static constexpr int V = V_W128;             using Cfg = W128Cfg;                static constexpr unsigned EPI = EPI_ALL & ~((1u << 2) | (1u << 3) | (1u << 6));      // plain long-K GEMMs: the transformer engines (GroupNorm partials take the general epilogue there)
                  template <int E> static constexpr auto kernel() { return &k_gemm_w128<E>; } };
using GemmFamilies = FamList<FamD128, FamRW4, FamR64, FamD256H, FamD512H, FamW128>;
using CfgR128x128 = RingCfg<2, 2, 4, 4, 4>;          // split-K only: k_gemm_ring<2, 2, 4, 4, 4, 9> (k_gemm_w128<9> is the four-wave tile's)

// f(Fam{}) for the family of variant id v; false when v is not a tile family (V_AUTO, V_GENERIC, V_FP8_256x256, V_CONV_GN, the retired ids)
template <class F, class... Fam> constexpr bool with_family(int v, F&& f, FamList<Fam...>) { return ((v == Fam::V && (f(Fam{}), true)) || ...); }
template <class F> constexpr bool with_family(int v, F&& f) { return with_family(v, f, GemmFamilies{}); }
constexpr bool variant_shipped(int v) {
    return v == V_AUTO || v == V_GENERIC || v == V_FP8_256x256 || v == V_CONV_GN || with_family(v, [](auto) {});
}
constexpr unsigned epi_mask(int v) { unsigned m = 1u; with_family(v, [&](auto f) { m = decltype(f)::EPI; }); return m; }
constexpr int variant_bm(int v) {
    int bm = (v == V_CONV_GN || v == V_FP8_256x256) ? 256 : 128;
    with_family(v, [&](auto f) { bm = decltype(f)::Cfg::BM_; });
    return bm;
}
static_assert(variant_bm(V_RING_64x128) == 64 && variant_bm(V_DMA_128x128_P) == 128 && variant_bm(V_RING_256x128_W4) == 256 && variant_bm(V_DMA_256x256_H) == 256 &&
              variant_bm(V_DMA_512x128_H) == 512 && variant_bm(V_W128) == 256 && variant_bm(V_GENERIC) == 128, "the block-tile rows choose_variant and the GroupNorm partial tables count on");
static_assert(variant_shipped(V_W128) && !variant_shipped(V_DMA_256x256) && !variant_shipped(V_W128_X) && epi_mask(V_GENERIC) == 1u, "retired ids stay refused");

// (2) the fused GroupNorm + SiLU + 3x3 convolution (conv_gn2.h): six tile shapes x the four packed epilogues it has
constexpr unsigned EPI_CONV_GN = (1u << 1) | (1u << 2) | (1u << 5) | (1u << 6);
template <int RES_, bool WIDE, int TM = 8, int NG = 1, int TN = 4> struct CgShape {
    static constexpr int RES = RES_; using Cfg = ConvGn2Cfg<RES_, WIDE, TM, NG, TN>; static constexpr unsigned EPI = EPI_CONV_GN;
    template <int E> static constexpr auto kernel() { return &k_conv_gn2<RES_, WIDE, E, TM, NG, TN>; }
    // 32x32 / 16x16: the 256 x 128 tile or the wide 128 x 256 one (conv_gn_bm); 8x8 / 4x4: one shape each
    // (the 8x8 level runs on 64-pixel x 256-channel tiles, one image per tile and two blocks per CU; the 128 x 256 tile with two images, natinf_set_conv_gn8_tile(0), is retired)
    static bool takes(int res, int bm) { return res == RES_ && (RES_ <= 8 || WIDE == (bm == 128)); }
};
using CgH4T = CgShape<4, true, 4, 2, 2>;
using ConvGnShapes = FamList<CgShape<32, false>, CgShape<32, true>, CgShape<16, false>, CgShape<16, true>, CgShape<8, true, 4>, CgH4T>;
template <class... S> void launch_conv_gn2(FamList<S...>, int res, int bm, int e, const GemmArgs& g, hipStream_t s) {
    ((S::takes(res, bm) && (launch_family<S>(e, g, s), true)) || ...);
}

// (2b) Conv_0 of the 16 -> 32 up-sampling res-block as four 2x2 phase convolutions over its 16x16 input (GemmArgs::taps == 4; up_fold.h, ncsn_upf): the hand-pipelined
// 256 x 256 tile -- one input image x one phase (256 output channels) -- with the packed epilogues 1 / 2 scattering to the phase's output parity
constexpr int UPFOLD_W = 16, UPFOLD_BM = UPFOLD_W * UPFOLD_W, UPFOLD_BN = 256;

// (3) fp8 operands: the eight-wave 256 x 256 tile (gemm_fp8.h) and the four-wave one (gemm_w128.h), each with plain or E8M0-scaled A x four epilogues
constexpr unsigned EPI_FP8 = 0xF;
template <bool MXA> struct FamF8     { using Cfg = CfgD256x256; static constexpr unsigned EPI = EPI_FP8; template <int E> static constexpr auto kernel() { return &k_gemm_fp8<MXA, E>; } };
template <bool MXA> struct FamF8W128 { using Cfg = W128F8Cfg;   static constexpr unsigned EPI = EPI_FP8; template <int E> static constexpr auto kernel() { return &k_gemm_w128_fp8<MXA, E>; } };
using Fp8Families = FamList<FamF8<false>, FamF8<true>, FamF8W128<false>, FamF8W128<true>>;

bool configure_gemm_kernels() {
    bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_bf16), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  GEMM_LDS_BYTES) == hipSuccess;
    ok = ok && set_lds<CfgR128x128>(&k_gemm_ring<2, 2, 4, 4, 4, 9>) && set_lds<W128Cfg>(&k_gemm_w128<9>) &&
         configure_families(GemmFamilies{}) && configure_families(ConvGnShapes{}) && ncsn_upf::configure() && configure_families(Fp8Families{}) &&
         ncsn_cg3::configure() && ncsn_sg::configure() && ::configure_conv_ring() && configure_ncsnpp_kernels() && configure_dit_attention() && configure_flash_attention();
    if (!ok) (void)hipGetLastError();
    return ok;
}

// Automatic choice: the largest block tile that still gives every CU a tile (DMA kernels need K a multiple of
// 64 per segment and zero-bordered 3x3 operands); the register-staged, fully masked kernel otherwise (4x4
// attention: K = 16).

int packed_epi(const GemmArgs& g, int bm);
int g_cg3 = 7;                     // natinf_set_conv_gn_w128: bit 0 = 32x32 layers with N % 256 != 0 on 512 x 128 tiles, bit 1 = 32x32 layers with N % 256 == 0 on 256 x 256
                                   // tiles, bit 2 = 16x16 layers with N % 256 == 0 on 256 x 256 tiles (one image per tile)
int g_cg_wide = 3;                 // natinf_set_conv_gn_wide: bit 0 = 128 x 256 tiles at 16x16, bit 1 = at 32x32 (N % 256 == 0 layers: the 16 -> 32 up-sampling block)
// tile rows of the fused-convolution instantiation a launch takes: 128 x 256 tiles at 16x16 (N % 256 == 0) and at 8x8 (two images per tile), 256 x 128 elsewhere
// the k_conv_gn3 shape a fused-convolution launch takes (-1: k_conv_gn2).  One block per CU exposes a tile's prologue and epilogue (~28k clocks), which the two
// co-resident blocks of k_conv_gn2 partly hide: k_conv_gn3 is ahead where the K loop is long (same-process A/B at B = 512, profiles/r05/cg3_v2_ab.log: 1.04-1.08 at
// K >= 2,304 on 512 x 128 tiles, 1.035-1.04 on 256 x 256 tiles at 32x32, 1.01-1.06 at K >= 2,816 at 16x16; inside the network, rocprofv3 trace of both in one process, profiles/r05/cg3_in_network_ab_by_shape.txt: 1.08-1.15 at K >= 2,304 at 32x32, 1.02-1.09 at K >= 2,304 at 16x16) and level or behind at short K (0.97-0.99 at K = 1,152 .. 1,536)
int g_cg3_min_k[3] = {2304, 0, 2304};      // natinf_set_conv_gn_w128_min_k: smallest K (9 cin + shortcut channels) per shape that takes k_conv_gn3
inline int conv_gn3_shape(const GemmArgs& g) {
    const int res = 1 << g.logW;
    if (!g_cg3 || !g.b_frag || g.N % 128) return -1;
    int sh = -1;
    if (res == 32) sh = g.N % 256 ? ((g_cg3 & 1) ? 0 : -1) : ((g_cg3 & 2) ? 1 : -1);
    else if (res == 16) sh = (g.N % 256 == 0 && (g_cg3 & 4)) ? 2 : -1;
    if (sh >= 0 && 9 * g.a0_C + (g.a1 ? g.a1_C : 0) < g_cg3_min_k[sh]) sh = -1;
    return sh;
}
inline int conv_gn_bm(const GemmArgs& g) {
    const int res = 1 << g.logW;
    if (const int sh3 = conv_gn3_shape(g); sh3 >= 0) return ncsn_cg3::tile_rows(sh3);
    if (res == 8 || res == 4) return 64;
    if (res == 32) return ((g_cg_wide & 2) && g.N % 256 == 0 && g.b_frag) ? 128 : 256;
    return ((g_cg_wide & 1) && res == 16 && g.N % 256 == 0) ? 128 : 256;
}
// rows of one GroupNorm-partial table row the launch writes (what the caller divides H*W by): a tile, or one SAMPLE of the two an 8x8 tile holds
inline int conv_gn_part_rows(const GemmArgs& g) { const int res = 1 << g.logW; return res <= 8 ? res * res : conv_gn_bm(g); }
inline bool conv_gn_regw(const GemmArgs& g) { return g.b_frag && (conv_gn3_shape(g) >= 0 || g.N % ((conv_gn_bm(g) <= 128 && (1 << g.logW) != 4) ? 256 : 128) == 0); }      // (4x4: 64 x 128 tiles)
// k_conv_gn2 / k_conv_gn3 have packed epilogues only: the fp32-slab A/B knob (natinf_set_gemm_epilogue) does not apply to them.  Per-sample terms need
// one sample per tile -- or, at 8x8, per HALF tile (the kernel keeps both samples' row vectors and partials: NSAMP)
inline int conv_gn_epi(const GemmArgs& g) { GemmArgs t = g; t.epi_fp32_slab = 0; return packed_epi(t, conv_gn_part_rows(g)); }
inline bool conv_gn_ok(const GemmArgs& g) {
    if (!g.gn_scale || !g.gn_shift || !g.gn_folded || g.taps != 9 || g.batch != 1 || g.a0_C % BK || (g.a1 && g.a1_C % BK)) return false;
    const int res = 1 << g.logW;
    if (g.logHW != 2 * g.logW || (res != 32 && res != 16 && res != 8 && res != 4) || g.N % 8) return false;
    if (res == 4 && (g.a0_C % (64 * CgH4T::Cfg::NG) || (g.a1 && g.a1_C % (64 * CgH4T::Cfg::NG)))) return false;          // two K groups per block: an even number of half-chunks / shortcut tiles EACH
    if (res <= 8 ? (g.M % (res * res) || g.N % (res == 4 ? 128 : 256) || g.a0_up || g.a1_up || (g.resid && g.rowvec)) : g.M % std::max(256, conv_gn_bm(g)) != 0) return false;      // 8x8 / 4x4: whole images;
    // (the residual epilogues keep one set of column terms for all samples of a tile: no per-sample row vector there)
    if (!conv_gn_regw(g)) return false;                                                       // the fragment-major weights, whole column tiles
    const int e = conv_gn_epi(g);
    return e == 1 || e == 2 || e == 5 || e == 6;
}
int g_w128 = 1;                     // natinf_set_gemm_w128(0): plain GEMMs on the two-waves-per-SIMD 256x256 tile as before round 4 (A/B runs)
// k_gemm_w128 (gemm_w128.h): plain GEMMs only, 32-bit lane offsets into the operands
bool w128_ok(const GemmArgs& g) {
    if (g.taps != 1 || g.a1 || g.gn_scale || g.deq_m || g.deq_n || g.splitk > 1) return false;
    if (g.a0_C % BK || g.a0_C < 2 * BK || g.N % 8 || g.M % 8) return false;
    return (int64_t)g.M * g.a0_ld * 2 < (int64_t)1 << 32 && (int64_t)g.N * g.b_ld * 2 < (int64_t)1 << 32;
}
int choose_variant(const GemmArgs& g) {
    if (g.gn_scale) return V_CONV_GN;               // the operand is raw: no other kernel can read it (launch_gemm checks conv_gn_ok)
    const int K0 = g.taps * g.a0_C, K1 = g.a1 ? g.a1_C : 0;
    const bool dma = K0 % BK == 0 && K1 % BK == 0 && (g.taps == 1 || (g.a0_padded && g.a0_C % BK == 0));
    if (!dma) return V_GENERIC;
    // (g_force_variant is always a shipped id: natinf_set_gemm_variant / natinf_debug_gemm refuse the others)
    if (g_force_variant == V_W128) {
        if (w128_ok(g) && (!g.gn_part || (1 << g.logHW) % 256 == 0)) return V_W128;
    }
    else if (g_force_variant > V_GENERIC && g_force_variant != V_CONV_GN && g_force_variant != V_FP8_256x256) {
        // a forced tile must keep GroupNorm partial tiles inside one sample (e.g. 512-row tiles on the 16x16 level do not): the launch has to say what a
        // sample is -- a 3x3 launch always does, a plain GEMM when its caller sets logHW (the im2col'ed stride-2 convolutions; the V_W128 rule above reads the same field)
        if (!g.gn_part || ((g.taps == 9 || g.logHW > 0) && (1 << g.logHW) % variant_bm(g_force_variant) == 0)) return g_force_variant;
    }
    // measured on the engine's layer shapes (tools/bench_gemm.py, profiles/r01): 256x256 two-stage for wide-N,
    // long-K layers; the 4-wave 256x128 ring (wave tile 128x64, 2 blocks/CU) for N = 128 and short-K layers;
    // 128x128 when 256-row tiles would leave CUs idle; 64x128 for the 4x4 level
    const int64_t mt256 = (g.M + 255) / 256, mt128 = (g.M + 127) / 128;
    const int64_t nt128 = (g.N + 127) / 128;
    const bool w128 = g_w128 && w128_ok(g) && (!g.gn_part || (1 << g.logHW) % 256 == 0);       // round 4: plain GEMMs on the one-wave-per-SIMD tile (gemm_w128.h)
    // Round 4: small-M plain GEMMs (the text stream of the MMDiT: M = 8 x 333 rows) by ROUNDS of blocks, not by "enough tiles for every CU": at
    // (2664, 6144, 1536) the rule below took 256 x 256 tiles -- 264 of them: a second round for eight tiles, 77 us -- where 1,008 tiles of 128 x 128 run as two rounds of
    // two blocks per CU in 55 us; at (2664, 4608, 1536) it took 128 x 128 (756 tiles, two rounds, 52 us) where 198 tiles of 256 x 256 are ONE round (43 us).  Measured
    // cost of a round at K = 1,536: 25-28 us (128 x 128, two blocks per CU) against 37-43 us (256 x 256): ratio 1.5 (tools/scan_small_m_gemm.py).
    // (round 5: the four-wave tile multiplies its 256 columns as two 128-column halves and skips a half that lies beyond N, so N % 128 == 0 is enough for it --
    // DiT-XL/2's q | k | v projection, N = 3,456 = 13.5 tiles, had fallen to 128 x 128 tiles: 50.7 us against 30 us)
    const int64_t nt256 = (g.N + 255) / 256;
    const bool n_ok256 = g.N % 256 == 0 || (w128 && g.N % 128 == 0);
    if (g_round_model && g.taps == 1 && !g.gn_part && g.batch == 1 && n_ok256 && K0 + K1 >= 1024 && mt256 * nt256 < 2 * NUM_CU) {
        const int64_t r256 = (mt256 * nt256 + NUM_CU - 1) / NUM_CU, r128 = (mt128 * nt128 + 2 * NUM_CU - 1) / (2 * NUM_CU);
        // (a round of the four-wave 256 x 256 tile costs ~1.3 rounds of 128 x 128 tiles, not 1.5: DiT-XL/2's fc1 at B = 16, (4096, 4608, 1152), is 288 tiles = two rounds of
        // ~28 us against three rounds of two 128 x 128 blocks per CU in 74.6 us; natinf_set_gemm_round_model(v >= 10) sets the ratio to v / 10 for A/B runs)
        const int64_t c256 = w128 ? g_round_model_w128 : 15;
        if (mt128 * nt128 >= NUM_CU / 2) return c256 * r256 < 10 * r128 ? (w128 ? V_W128 : V_DMA_256x256_H) : V_DMA_128x128_P;
    }
    if (n_ok256 && K0 + K1 >= 1024 && mt256 * nt256 * g.batch >= NUM_CU) return w128 ? V_W128 : V_DMA_256x256_H;
    if (g_pref_512 && g.N <= 128 && K0 + K1 >= 1024 && ((g.M + 511) / 512) * g.batch >= 2 * NUM_CU &&
        (!g.gn_part || (g.taps == 9 && (1 << g.logHW) % 512 == 0)))           // GroupNorm partials: a tile inside one sample
        return V_DMA_512x128_H;
    if (mt256 * nt128 * g.batch >= 2 * NUM_CU) return V_RING_256x128_W4;        // it runs two blocks per CU
    if (mt128 * nt128 * g.batch >= NUM_CU) return V_DMA_128x128_P;
    return V_RING_64x128;
}

// fp8 operands (a0 / b point at e4m3 bytes, a0_ld / b_ld / a_bs / b_bs in bytes, a0_C = K % 128 == 0, deq_m / deq_n set)
int fp8_epi(const GemmArgs& g) {
    if (g.epi_fp32_slab || g.resid || g.gn_part) return 0;
    if ((g.rowvec || g.gate) && g.log_rows_per_sample < 30 && ((1 << g.log_rows_per_sample) % 256 != 0)) return 0;
    if (g.c_mode == OUT_F32 && g.resid_f32 && !g.bias_m && g.act == ACT_NONE && g.resid_f32_ld % 4 == 0 && g.c_ld % 4 == 0) return 3;
    if (g.resid_f32 || g.gate) return 0;
    if (g.c_mode == OUT_BF16 && g.act == ACT_NONE) return 1;
    if (g.c_mode == OUT_FP8_MX && g.act == ACT_GELU_TANH && g.c_mx && g.N % 32 == 0 && !g.bias_m && g.scale == 1.0f) return 2;      // (its epilogue carries neither term)
    return 0;
}
// k_gemm_w128_fp8 (gemm_w128.h): an even number of 128-byte K-tiles, 32-bit offsets into the operands
// (DiT-XL/2's K = 1,152 is NINE K-tiles: an odd-count form of the four-wave kernel -- the parity kept a template parameter, one more steady-state iteration and the two
// closing iterations on swapped stages; no spill, same bytes -- was measured against the eight-wave tile in one process and not kept, TFLOP/s four-wave / eight-wave:
// (4096, 3456, 1152) -> bf16 1,391 / 1,384, (4096, 1152, 1152) 539 / 582, (4096, 4608, 1152) GELU -> e4m3 + E8M0 875 / 885; at M = 8,192 1,479 / 1,478, 990 / 1,010, 1,115 / 1,140;
// at M = 32,768 1,683 / 1,683, 1,388 / 1,386, 1,464 / 1,475: level or behind on every shape -- nine K-tiles are too short a loop for the one-wave-per-SIMD schedule to earn
// back its longer prologue and epilogue.  Those GEMMs run on k_gemm_fp8; profiles/dit_fp8/ab_k1152.txt)
bool w128_fp8_ok(const GemmArgs& g) {
    // (E8M0 block scales of A arrive by DMA as whole 256-row groups per K-tile: the plane must hold them -- whole row tiles only)
    return g.taps == 1 && !g.a1 && g.a0_C % 256 == 0 && g.N % 8 == 0 && g.M % 8 == 0 && (!g.a_mx || g.M % 256 == 0) &&
           (int64_t)g.M * g.a0_ld < (int64_t)1 << 32 && (int64_t)g.N * g.b_ld < (int64_t)1 << 32;
}
bool fp8_on_w128(const GemmArgs& g) { return g_w128 && w128_fp8_ok(g) && (fp8_epi(g) != 2 || g_w128 != 2); }      // the four-wave tile takes this launch
template <bool MXA>
void launch_gemm_fp8_t(const GemmArgs& g, hipStream_t s) {
    // (round 5: the e4m3 + E8M0 epilogue with its tanh-GELU -- fc1 -- takes the four-wave tile too: with the GELU issued stage by stage for eight values at a time
    // (gelu_tanh_fast8) (32768, 6144, 1536) runs 1,756-1,759 TFLOP/s there against 1,641-1,697 on the eight-wave tile, same process (tools/ab_fc1_w128.py).  Round 4 kept it on
    // the eight-wave tile on a figure -- 1,100-1,130 against 1,300-1,520 -- that the debug entry had measured on the fp32-SLAB epilogue in e4m3 mode (no activation
    // passed: fp8_epi() = 0), not on this one.  natinf_set_gemm_w128(2) = the round-4 rule, for A/B runs.)
    if (fp8_on_w128(g)) launch_family<FamF8W128<MXA>>(fp8_epi(g), g, s);
    else launch_family<FamF8<MXA>>(fp8_epi(g), g, s);
}
// one row of natinf_ncsnpp_describe_gemms, also the tag of a natinf_gemm_profile record: "M N K0 K1 taps batch name/eE"
std::string gemm_row(int M, int N, int K0, int K1, int taps, int batch, const std::string& name, int epi) {
    char line[160];
    snprintf(line, sizeof(line), "%d %d %d %d %d %d %s/e%d", M, N, K0, K1, taps, batch, name.c_str(), epi);
    return line;
}
void record_gemm(const GemmArgs& g, const std::string& name, int epi) { *g_record += gemm_row(g.M, g.N, g.taps * g.a0_C, g.a1 ? g.a1_C : 0, g.taps, g.batch, name, epi) + "\n"; }
// natinf_gemm_profile(1): every matmul-shaped launch of every engine -- launch_gemm and launch_gemm_fp8, i.e. the kernel WITH the epilogue it runs in the network, on
// the stream it runs on, between its real neighbours -- is bracketed by a HIP event pair and tagged with the line natinf_ncsnpp_describe_gemms would print for it.
// natinf_gemm_profile_read sums them per tag.  (Round-5 review, item 2: the SD3 bench line quoted isolated loops of debug entries with the plain epilogue.)
// One host thread at a time, like natinf_attention_profile; the events serialise nothing, but two HIP streams still overlap: a launch's span then includes what it
// shared the chip with -- bench.py reads the image-stream shapes, whose launches are 10-100x the text stream's.
struct GemmProf {
    struct Rec { hipEvent_t a, b; std::string tag; };
    bool on = false; std::vector<Rec> ev; std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    bool begin(Rec& r, hipStream_t s) {
        r.a = r.b = nullptr;
        if (!pool.empty()) { r.a = pool.back().first; r.b = pool.back().second; pool.pop_back(); }
        else if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) { r.a = r.b = nullptr; (void)hipGetLastError(); return false; }
        (void)hipEventRecord(r.a, s);
        return true;
    }
    void end(Rec& r, hipStream_t s) { (void)hipEventRecord(r.b, s); ev.push_back(std::move(r)); }
} g_gemm_prof;
thread_local int g_launch_error = 0;
void launch_gemm_fp8(const GemmArgs& g, hipStream_t s) {
    if (g.stream_guard && fp8_epi(g) != 3) { g_launch_error = 1; return; }      // only the direct residual epilogue has a guarded form: never an unguarded write of a guarded site
    GemmProf::Rec r;
    const bool prof = g_gemm_prof.on && !g_record && g_gemm_prof.begin(r, s);
    if (prof) r.tag = gemm_row(g.M, g.N, g.taps * g.a0_C, 0, g.taps, g.batch, std::string(fp8_on_w128(g) ? "w128_fp8" : "fp8_256x256") + (g.a_mx ? "_mxa" : ""), g.stream_guard ? 4 : fp8_epi(g));
    if (g.stream_guard) ncsn_sg::launch_fp8(&g, g.a_mx != nullptr, fp8_on_w128(g), g_raster_g, (void*)s);      // the same tile, EPI 4
    else if (g.a_mx) launch_gemm_fp8_t<true>(g, s); else launch_gemm_fp8_t<false>(g, s);
    if (prof) g_gemm_prof.end(r, s);
}

// Which epilogue a launch can take (see tile_epilogue in gemm_dma.h): 0 = the general fp32-slab one; 1..6 = packed, when only
// column terms (bias, a per-sample row vector with every block tile inside one sample) and a bf16 residual are fused, the output is bf16, and
// GroupNorm partials (no activation, whole tiles) or an activation -- not both -- are asked for.
int packed_epi(const GemmArgs& g, int bm) {      // resid must be 8-byte aligned per 4-column group: ld % 4, base from the arena
    if (g.epi_fp32_slab || g.deq_m || g.deq_n || g.act == ACT_RELU) return 0;      // (ReLU: the general epilogue applies it)
    if (g.bias_m) return (g.c_mode == OUT_BF16 && !g.resid && !g.resid_f32 && !g.gate && !g.rowvec && !g.gn_part && g.act == ACT_NONE) ? 8 : 0;
    if ((g.rowvec || g.gate) && g.log_rows_per_sample < 30 && ((1 << g.log_rows_per_sample) % bm != 0)) return 0;    // per-sample terms: one sample per tile
    if (g.c_mode == OUT_F32 && g.resid_f32 && !g.resid && !g.gn_part && g.act == ACT_NONE && g.resid_f32_ld % 4 == 0 && g.c_ld % 4 == 0) return 7;
    if (g.c_mode != OUT_BF16 || g.resid_f32 || g.gate) return 0;
    if (g.resid && (g.act != ACT_NONE || g.resid_ld % 4 != 0)) return 0;
    if (g.gn_part) return (g.act == ACT_NONE && g.M % bm == 0) ? (g.resid ? 6 : 2) : 0;
    if (g.resid) return 5;
    return g.act == ACT_NONE ? 1 : (g.act == ACT_SILU ? 3 : 4);
}
// the epilogue specialization a launch on tile variant v runs (0 where its packed one is not instantiated for that tile)
inline int effective_epi(int v, const GemmArgs& g) { const int e = packed_epi(g, variant_bm(v)); return ((epi_mask(v) >> e) & 1u) ? e : 0; }

// set when a launch is asked for something no kernel provides (a plan-builder bug, or an A/B knob flipped after the plan was built);
// natinf_ncsnpp_forward clears it on entry and reports it on exit -- per calling thread, so two engines on two threads do not see
// each other's, and a description pass (g_record) never sets it (g_launch_error: declared in front of launch_gemm_fp8; guarded engines check it too, EngineCore::run)
thread_local bool g_fin_written = false;      // set by launch_gemm: the launch that just ran wrote the consumer's GroupNorm table (GemmArgs::fin_*) -- k_conv_gn3 at 16x16
int g_splitk = 1;                  // natinf_set_gemm_splitk: 0 = never split K
float* g_dbg_splitk_ws = nullptr; int g_dbg_splitk_max = 0;        // natinf_debug_set_splitk_workspace
// Split-K for launches that cannot fill the chip otherwise (the 8x8 and 4x4 levels: 32,768 / 8,192 rows x 256 columns, K = 2,304 ..
// 4,608): 128 x 128 tiles (fill per flop of the large tile) x S slices of K >= 2 blocks per CU, then one reduce pass with the fused
// terms.  Returns the slice count (1 = do not split).
int splitk_slices(const GemmArgs& g) {
    if (!g_splitk || !g.splitk_ws || g.splitk_max < 2 || g.batch != 1 || g.gn_scale || g.c_mode != OUT_BF16 || g.N % 8 || 256 % (g.N / 8)) return 1;
    if (g.gn_part && (g.M % SPLITK_ROWS || g.act != ACT_NONE || (g.taps == 9 && (1 << g.logHW) % SPLITK_ROWS))) return 1;
    if (g.bias_m || g.gate || g.resid_f32 || g.deq_m || g.deq_n) return 1;
    const int K0 = g.taps * g.a0_C, K1 = g.a1 ? g.a1_C : 0;
    if (K0 % 64 || K1 % 64 || (g.taps == 9 && !g.a0_padded) || K0 + K1 < 2048) return 1;
    const int64_t tiles = ((g.M + 127) / 128) * ((g.N + 127) / 128);
    if (tiles >= 2 * NUM_CU) return 1;
    int S = (int)((2 * NUM_CU + tiles - 1) / tiles);
    if (S > g.splitk_max) S = g.splitk_max;
    while (S > 1 && (K0 + K1) / 32 / S < 16) --S;                       // at least 16 K-tiles per slice
    return S;
}
// Split-K on the four-wave tile for under-filled long-K GEMMs with the gated fp32 residual epilogue (gemm_w128.h: k_gemm_w128<9> + k_splitk_reduce_f32).  Returns the
// slice count (1 = do not split): the tiles of 256 x 256 fill less than half the chip, every slice keeps >= 16 K-tiles.
int w128_splitk_slices(const GemmArgs& g) {
    // (batch 1 only: the workspace contract is splitk_max * M * N floats; a batched launch would need batch times that)
    if (!g_splitk || !g_w128 || !g.splitk_ws || g.splitk_max < 2 || g.batch != 1 || !w128_ok(g) || g.a0_C < 3072) return 1;
    if (g.c_mode != OUT_F32 || !g.resid_f32 || g.resid || g.rowvec || g.bias_m || g.gn_part || g.act != ACT_NONE || g.epi_fp32_slab || g.N % 4 || g.c_ld % 4 || g.resid_f32_ld % 4) return 1;
    const int64_t tiles = (int64_t)((g.M + 255) / 256) * ((g.N + 255) / 256) * g.batch;
    if (tiles * 2 > NUM_CU) return 1;
    int S = (int)(NUM_CU / tiles);
    if (S > g.splitk_max) S = g.splitk_max;
    while (S > 1 && g.a0_C / BK / S < 16) --S;
    return S;
}
int launch_gemm_run(const GemmArgs& g0, hipStream_t s);
// returns the block-tile row count of the variant used
int launch_gemm(const GemmArgs& g0, hipStream_t s) {
    if (!g_gemm_prof.on || g_record) return launch_gemm_run(g0, s);
    GemmProf::Rec r;
    std::string tag;
    g_record = &tag; (void)launch_gemm_run(g0, s); g_record = nullptr;          // description pass: the tag, nothing launched
    while (!tag.empty() && tag.back() == '\n') tag.pop_back();
    if (!g_gemm_prof.begin(r, s)) return launch_gemm_run(g0, s);
    r.tag = std::move(tag);
    const int bm = launch_gemm_run(g0, s);
    g_gemm_prof.end(r, s);
    return bm;
}
// the up-fold launch (ncsn_upf::launch): the zero-bordered activated 16x16 input, N = 4 phases x 256 channels, column terms and GroupNorm partials only.  Returns its epilogue, 0 = not one
inline int up_fold_epi(const GemmArgs& g) {
    if (g.taps != 4 || !g.a0_padded || g.a1 || g.gn_scale || g.batch != 1 || g.logW != 4 || g.logHW != 8 || g.log_rows_per_sample != 8 || g.a0_C <= 0 || g.a0_C % BK ||
        g.N != 4 * UPFOLD_BN || g.M <= 0 || g.M % UPFOLD_BM || g.b_ld != 4 * g.a0_C || g.resid || g.c_ld % 8) return 0;
    GemmArgs t = g; t.epi_fp32_slab = 0;
    const int e = packed_epi(t, UPFOLD_BM);
    return (e == 1 || e == 2) ? e : 0;
}
int launch_gemm_run(const GemmArgs& g0, hipStream_t s) {
    if (g0.taps == 4) {
        // four phase tiles per sample = four GroupNorm partial rows per sample of the 32x32 output: 256 output pixels per row
        const int e = up_fold_epi(g0);
        if (!e) { if (g_record) record_gemm(g0, "invalid_conv_gn_upfold", 0); else g_launch_error = 1; return 256; }
        if (g_record) { record_gemm(g0, "conv_gn_upfold", e); return 256; }      // the ISSUED shape: low-resolution M, N = 4 x 256, K = 4 cin
        ncsn_upf::launch(&g0, e, (void*)s);
        return 256;
    }
    if (g_force_variant == V_AUTO) {
        const int S8 = w128_splitk_slices(g0);
        if (S8 > 1) {
            if (g_record) { record_gemm(g0, "splitk" + std::to_string(S8) + "_w128_256x256", 7); return 256; }      // (w128_ok: no second operand, K1 = 0)
            GemmArgs p = g0;
            p.splitk = S8; p.c = g0.splitk_ws; p.c_mode = OUT_F32;
            const int nM = (p.M + 255) / 256, nN = (p.N + 255) / 256;
            p.raster_g = 0;
            hipLaunchKernelGGL((k_gemm_w128<9>), dim3(nM * nN, S8, p.batch), dim3(256), W128Cfg::LDS_BYTES, s, p);
            if (g0.stream_guard) ncsn_sg::launch_splitk_reduce(&g0, S8, (void*)s);
            else launch_splitk_reduce_f32<false>(g0, S8, s);
            return 256;
        }
    }
    const int S = g_force_variant == V_AUTO ? splitk_slices(g0) : 1;
    if (S > 1) {
        if (g_record) { record_gemm(g0, "splitk" + std::to_string(S) + "_ring128x128", 9); return SPLITK_ROWS; }
        GemmArgs p = g0;
        p.splitk = S; p.c = g0.splitk_ws; p.c_mode = OUT_F32; p.batch = S;
        p.bias_n = nullptr; p.rowvec = nullptr; p.resid = nullptr; p.scale = 1.0f; p.act = ACT_NONE; p.gn_part = nullptr;
        launch_tiles<CfgR128x128>(&k_gemm_ring<2, 2, 4, 4, 4, 9>, p, s);
        hipLaunchKernelGGL(k_splitk_reduce, dim3((unsigned)((g0.M + SPLITK_ROWS - 1) / SPLITK_ROWS)), dim3(256), 0, s, g0.splitk_ws, S, g0.M, g0.N,
                           g0.bias_n, g0.rowvec, g0.rowvec_ld, g0.log_rows_per_sample, reinterpret_cast<const bf16*>(g0.resid), g0.resid_ld, g0.scale,
                           g0.act, reinterpret_cast<bf16*>(g0.c), g0.c_ld, reinterpret_cast<float2*>(g0.gn_part), g0.gn_quads);
        return SPLITK_ROWS;
    }
    const GemmArgs& g = g0;
    const int v = choose_variant(g);
    if (g.taps == 9 && v != V_CONV_GN && g.a0_C % BK) {
        // (the packed weight rows of a 3x3 launch hold ((c / 64) * 9 + tap) * 64 + c % 64 columns: with a0_C % 64 != 0 no kernel has a defined K order)
        if (g_record) record_gemm(g, "invalid_conv3x3", 0); else g_launch_error = 1;
        return 256;
    }
    if (v == V_CONV_GN && !conv_gn_ok(g)) {
        if (g_record) record_gemm(g, "invalid_conv_gn", 0); else g_launch_error = 1;      // description pass: say so in the table instead of dropping the row
        return 256;
    }
    const bool guarded = g.stream_guard != nullptr;      // the same tile with EPI 10 in place of 7 (stream_guard.hip); anything else is refused: no unguarded write of a guarded site
    if (guarded && !g_record && (!ncsn_sg::has_tile(v) || effective_epi(v, g) != 7)) { g_launch_error = 1; return 256; }
    if (g_record) {
        record_gemm(g, v == V_CONV_GN && conv_gn3_shape(g) >= 0 ? "conv_gn3" : variant_name(v), v == V_CONV_GN ? conv_gn_epi(g) : (guarded && effective_epi(v, g) == 7 ? 10 : effective_epi(v, g)));
        return v == V_CONV_GN ? conv_gn_part_rows(g) : variant_bm(v);
    }
    if (guarded) ncsn_sg::launch_tile(&g, v, g_raster_g, (void*)s);
    else if (v == V_GENERIC) {
        const int nM = (g.M + BM - 1) / BM, nN = (g.N + BN - 1) / BN;
        hipLaunchKernelGGL(k_gemm_bf16, dim3(nM * nN, 1, g.batch), dim3(256), GEMM_LDS_BYTES, s, g);
    } else if (v == V_CONV_GN) {
        GemmArgs gw = g0;
        gw.w_warm = (g_cg_warm >> (g0.logW - 2)) & 1;
        const int e = conv_gn_epi(gw);
        if (const int sh3 = conv_gn3_shape(gw); sh3 >= 0) {
            ncsn_cg3::launch(&gw, sh3, e, (void*)s);
            g_fin_written = sh3 == 2 && gw.fin_scale && (e == 2 || e == 6) && gw.N == 256;      // (k_conv_gn3<16, 2, 2, 2 | 6>: FIN16, conv_gn3.h)
        } else launch_conv_gn2(ConvGnShapes{}, 1 << gw.logW, conv_gn_bm(gw), e, gw, s);
        return conv_gn_part_rows(gw);
    } else with_family(v, [&](auto f) { launch_family<decltype(f)>(effective_epi(v, g), g, s); });
    return variant_bm(v);
}
inline int grid1d(int64_t n, int block = 256, int cap = 4096) {
    int64_t g = (n + block - 1) / block; return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace
