// up_fold.hip -- the kernels of natinf_set_fuse_up_fold (up_fold.h) in a translation unit of their own, like conv_gn3.hip: the shared kernel headers are included into
// an anonymous namespace (internal linkage), the interface to ncsnpp.hip is three plain functions that take the launch arguments as bytes (the same GemmArgs layout).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace {
#include "up_fold.h"
}
using namespace ncsn;

namespace ncsn_upf {
__attribute__((visibility("hidden"))) bool configure() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv_gn_upfold<1>), hipFuncAttributeMaxDynamicSharedMemorySize, UpFoldCfg::LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv_gn_upfold<2>), hipFuncAttributeMaxDynamicSharedMemorySize, UpFoldCfg::LDS_BYTES) == hipSuccess;
}
// epi: 1 (plain packed epilogue) or 2 (+ GroupNorm partials); M = whole 16x16 images, N = 4 phases x 256 channels (launch_gemm checks: up_fold_epi)
__attribute__((visibility("hidden"))) void launch(const void* gemm_args, int epi, void* stream) {
    GemmArgs g;
    memcpy(&g, gemm_args, sizeof(g));
    g.raster_g = 0;                                       // row-major tiles: the four phases of an image follow each other (its patch stays in L2)
    const dim3 grid((unsigned)((g.M / UpFoldCfg::BM_) * (g.N / UpFoldCfg::BN_)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (epi == 2) hipLaunchKernelGGL((k_conv_gn_upfold<2>), grid, dim3(UpFoldCfg::THREADS), UpFoldCfg::LDS_BYTES, s, g);
    else hipLaunchKernelGGL((k_conv_gn_upfold<1>), grid, dim3(UpFoldCfg::THREADS), UpFoldCfg::LDS_BYTES, s, g);
}
__attribute__((visibility("hidden"))) void fold(const float* w, void* dst_bf16, float* dst_f32, int N, int Cin, float wmul, void* stream) {
    const int64_t n = (int64_t)N * Cin;
    hipLaunchKernelGGL(k_fold_up_conv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), w, reinterpret_cast<bf16*>(dst_bf16), dst_f32, N, Cin, wmul);
}
}  // namespace ncsn_upf
