// stream_guard.hip -- the guarded forms of every kernel that writes a transformer engine's residual stream (include/natinf_dit.h, NATINF_DIT_STREAM_GUARD), in a
// translation unit of their own, as conv_gn3.hip is: ncsnpp.hip already takes the longest of the build, and its instance lists (gemm_launch.h) stay the unguarded library's.
// What a guard does is stated in ncsnpp_kernels.h (stream_guard_value / stream_guard_commit); the epilogue that carries it is gemm_dma.h's direct_f32_epilogue<..., GUARD>.
// No kernel body lives here: the split-K reduce (gemm_w128.h: k_splitk_reduce_f32<GUARD>) and the patch embedding (transformer_rows.h: k_patch_embed<XH, GUARD>) are the
// unguarded kernels' templates, instantiated here with GUARD = true.  The shared kernel headers define non-template kernels, so they are included into an anonymous namespace (internal linkage); the interface to ncsnpp.hip is plain
// functions that take the launch arguments as bytes (the same GemmArgs layout: the same header).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include <utility>

namespace {
#include "gemm_w128.h"
#include "gemm_fp8.h"
#include "transformer_rows.h"
}  // namespace
using namespace ncsn;

namespace {
// the bf16 tile families that have the direct residual epilogue (gemm_launch.h: GemmFamilies, by variant id), here with EPI 10 in place of 7
struct SgD128  { static constexpr int V = 17; using Cfg = DmaCfg<2, 2, 4, 4>;     static constexpr auto kernel() { return &k_gemm_dma<2, 2, 4, 4, 2, 10>; } };
struct SgRW4   { static constexpr int V = 9;  using Cfg = RingCfg<2, 2, 8, 4, 3>; static constexpr auto kernel() { return &k_gemm_ring<2, 2, 8, 4, 3, 10>; } };
struct SgR64   { static constexpr int V = 8;  using Cfg = RingCfg<2, 2, 2, 4, 4>; static constexpr auto kernel() { return &k_gemm_ring<2, 2, 2, 4, 4, 10>; } };
struct SgD256H { static constexpr int V = 26; using Cfg = DmaCfg<2, 4, 8, 4>;     static constexpr auto kernel() { return &k_gemm_dma<2, 4, 8, 4, 6, 10>; } };
struct SgW128  { static constexpr int V = 29; using Cfg = W128Cfg;                static constexpr auto kernel() { return &k_gemm_w128<10>; } };
template <bool MXA> struct SgF8     { using Cfg = DmaCfg<2, 4, 8, 4>; static constexpr auto kernel() { return &k_gemm_fp8<MXA, 4>; } };
template <bool MXA> struct SgF8W128 { using Cfg = W128F8Cfg;          static constexpr auto kernel() { return &k_gemm_w128_fp8<MXA, 4>; } };

template <class F> bool set_lds() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(F::kernel()), hipFuncAttributeMaxDynamicSharedMemorySize, F::Cfg::LDS_BYTES) == hipSuccess;
}
template <class F> void launch(GemmArgs g, int raster, hipStream_t s) {          // gemm_launch.h: launch_tiles
    const int nM = (g.M + F::Cfg::BM_ - 1) / F::Cfg::BM_, nN = (g.N + F::Cfg::BN_ - 1) / F::Cfg::BN_;
    g.raster_g = (raster > 1 && nN >= 8 && nM >= raster) ? raster : 0;
    hipLaunchKernelGGL(F::kernel(), dim3(nM * nN, 1, g.batch), dim3(F::Cfg::THREADS), F::Cfg::LDS_BYTES, s, g);
}
GemmArgs args_of(const void* p) { GemmArgs g; memcpy(&g, p, sizeof(g)); return g; }
}  // namespace

namespace ncsn_sg {
#define NATINF_SG_HIDDEN __attribute__((visibility("hidden")))
NATINF_SG_HIDDEN bool configure() {
    return set_lds<SgD128>() && set_lds<SgRW4>() && set_lds<SgR64>() && set_lds<SgD256H>() && set_lds<SgW128>() &&
           set_lds<SgF8<false>>() && set_lds<SgF8<true>>() && set_lds<SgF8W128<false>>() && set_lds<SgF8W128<true>>();
}
NATINF_SG_HIDDEN bool has_tile(int v) { return v == SgD128::V || v == SgRW4::V || v == SgR64::V || v == SgD256H::V || v == SgW128::V; }
NATINF_SG_HIDDEN void launch_tile(const void* gemm_args, int v, int raster, void* stream) {
    const GemmArgs g = args_of(gemm_args);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (v == SgD128::V) launch<SgD128>(g, raster, s);
    else if (v == SgRW4::V) launch<SgRW4>(g, raster, s);
    else if (v == SgR64::V) launch<SgR64>(g, raster, s);
    else if (v == SgD256H::V) launch<SgD256H>(g, raster, s);
    else if (v == SgW128::V) launch<SgW128>(g, raster, s);
}
NATINF_SG_HIDDEN void launch_fp8(const void* gemm_args, int mxa, int w128, int raster, void* stream) {
    const GemmArgs g = args_of(gemm_args);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (w128) { if (mxa) launch<SgF8W128<true>>(g, raster, s); else launch<SgF8W128<false>>(g, raster, s); }
    else if (mxa) launch<SgF8<true>>(g, raster, s);
    else launch<SgF8<false>>(g, raster, s);
}
NATINF_SG_HIDDEN void launch_splitk_reduce(const void* gemm_args, int slices, void* stream) {      // behind k_gemm_w128<9> (gemm_launch.h: w128_splitk_slices)
    launch_splitk_reduce_f32<true>(args_of(gemm_args), slices, reinterpret_cast<hipStream_t>(stream));      // k_splitk_reduce_f32<true> (gemm_w128.h)
}
NATINF_SG_HIDDEN void launch_patch_embed(const float* z, const float* Wt, const float* bias, const float* pos, float* x, int C, int g, int D, int64_t rows, int x_f16, uint32_t* guard,
                                         void* stream) {
    launch_patch_embed_as<true>(z, Wt, bias, pos, x, C, g, D, rows, x_f16 != 0, guard, reinterpret_cast<hipStream_t>(stream));      // k_patch_embed<., true> (transformer_rows.h)
}
}  // namespace ncsn_sg
