// stream_guard.hip -- the guarded forms of every kernel that writes a transformer engine's residual stream (include/natinf_dit.h, NATINF_DIT_STREAM_GUARD), in a
// translation unit of their own, as conv_gn3.hip is: ncsnpp.hip already takes the longest of the build, and its instance lists (gemm_launch.h) stay the unguarded library's.
// What a guard does is stated in ncsnpp_kernels.h (stream_guard_value / stream_guard_commit); the epilogue that carries it is gemm_dma.h's direct_f32_epilogue<..., GUARD>.
// The shared kernel headers define non-template kernels, so they are included into an anonymous namespace (internal linkage); the interface to ncsnpp.hip is plain
// functions that take the launch arguments as bytes (the same GemmArgs layout: the same header).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include <utility>

namespace {
#include "gemm_w128.h"
#include "gemm_fp8.h"
namespace ncsn {
// The guarded form (GemmArgs::stream_guard; ncsnpp_kernels.h): the same sums in the same order, every value through stream_guard_value before it is stored, one commit
// per wave.  No lane leaves before the commit (the wave reduction reads all 64): a lane past the end computes nothing and contributes zeros.
__global__ __launch_bounds__(256) void k_splitk_reduce_f32_guard(const float* __restrict__ part, int S, int64_t slice_stride, int M, int N, const float* __restrict__ bias_n,
                                                                  const float* __restrict__ gate, int gate_ld, int log_rows_per_sample, int z_samples,
                                                                  const float* resid, int resid_ld, int64_t c_bs, float scale, float* c, int c_ld, int stream_f16, uint32_t* guard)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, per = (int64_t)M * (N >> 2);
    const int z = blockIdx.y;
    StreamGuardAcc ga;
    if (idx < per) {
        const int m = (int)(idx / (N >> 2)), n = (int)(idx - (int64_t)m * (N >> 2)) * 4;
        const float* p = part + ((int64_t)z * M + m) * N + n;
        f32x4 v = *reinterpret_cast<const f32x4*>(p);
        for (int sl = 1; sl < S; ++sl) { const f32x4 u = *reinterpret_cast<const f32x4*>(p + sl * slice_stride); v += u; }
        if (bias_n) { const f32x4 b = *reinterpret_cast<const f32x4*>(bias_n + n); v += b; }
        if (gate) { const f32x4 gt = *reinterpret_cast<const f32x4*>(gate + (int64_t)((m >> log_rows_per_sample) + z * z_samples) * gate_ld + n); v *= gt; }
        typedef _Float16 f16x4_sk __attribute__((ext_vector_type(4)));
        if (stream_f16) {
            if (resid) {
                const f16x4_sk rs = *reinterpret_cast<const f16x4_sk*>(reinterpret_cast<const _Float16*>(resid) + (int64_t)z * c_bs + (int64_t)m * resid_ld + n);
                v += f32x4{(float)rs[0], (float)rs[1], (float)rs[2], (float)rs[3]};
            }
            v *= scale;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = stream_guard_value<true>(ga, v[e]);
            const f16x4_sk o = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
            *reinterpret_cast<f16x4_sk*>(reinterpret_cast<_Float16*>(c) + (int64_t)z * c_bs + (int64_t)m * c_ld + n) = o;
        } else {
            if (resid) { const f32x4 rs = *reinterpret_cast<const f32x4*>(resid + (int64_t)z * c_bs + (int64_t)m * resid_ld + n); v += rs; }
            v *= scale;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = stream_guard_value<false>(ga, v[e]);
            *reinterpret_cast<f32x4*>(c + (int64_t)z * c_bs + (int64_t)m * c_ld + n) = v;
        }
    }
    stream_guard_commit(ga, guard);
}


constexpr int PE_TOK = 16;          // as dit_engine.inc
// The guarded form (NATINF_DIT_STREAM_GUARD / NATINF_MMDIT_STREAM_GUARD: site 0 of the status block; ncsnpp_kernels.h states the guard): the same sums in the same
// order, every value through stream_guard_value before it is stored.  D % 64 == 0, so a wave is past D as a whole or not at all: the waves that stay commit with 64 lanes.
template <bool XH>
__global__ __launch_bounds__(256) void k_patch_embed_guard(const float* __restrict__ z, const float* __restrict__ Wt, const float* __restrict__ bias, const float* __restrict__ pos,
                                                           float* __restrict__ x, int C, int g, int D, int64_t rows, uint32_t* __restrict__ guard)
{
    __shared__ float sp[PE_TOK][64];
    lds_poison();
    const int K = C * 4, T = g * g, S = 2 * g;
    const int64_t row0 = (int64_t)blockIdx.y * PE_TOK;
    const int d = blockIdx.x * 256 + threadIdx.x;
    for (int e = threadIdx.x; e < PE_TOK * K; e += 256) {
        const int tk = e / K, k = e - tk * K, c = k >> 2, pi = (k >> 1) & 1, qi = k & 1;
        const int64_t row = min(row0 + tk, rows - 1);
        const int t = (int)(row % T), gh = t / g, gw = t - gh * g; const int64_t b = row / T;
        sp[tk][k] = z[(((int64_t)b * C + c) * S + gh * 2 + pi) * S + gw * 2 + qi];
    }
    __syncthreads();
    if (d >= D) return;
    float acc[PE_TOK];
    const float bv = bias[d];
#pragma unroll
    for (int tk = 0; tk < PE_TOK; ++tk) acc[tk] = bv;
    for (int k = 0; k < K; ++k) {
        const float w = Wt[(int64_t)k * D + d];
#pragma unroll
        for (int tk = 0; tk < PE_TOK; ++tk) acc[tk] += w * sp[tk][k];
    }
    StreamGuardAcc ga;
#pragma unroll
    for (int tk = 0; tk < PE_TOK; ++tk) {
        const int64_t row = row0 + tk;
        if (row < rows) {
            const float v = stream_guard_value<XH>(ga, acc[tk] + pos[(row % T) * D + d]);
            if constexpr (XH) reinterpret_cast<_Float16*>(x)[row * D + d] = (_Float16)v; else x[row * D + d] = v;
        }
    }
    stream_guard_commit(ga, guard);
}
}  // namespace ncsn
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
    const GemmArgs g = args_of(gemm_args);
    const int64_t per = (int64_t)g.M * (g.N / 4);
    hipLaunchKernelGGL(k_splitk_reduce_f32_guard, dim3((unsigned)((per + 255) / 256), (unsigned)g.batch), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g.splitk_ws, slices,
                       (int64_t)g.batch * g.M * g.N, g.M, g.N, g.bias_n, g.gate, g.gate_ld, g.log_rows_per_sample, g.z_samples, g.resid_f32, g.resid_f32_ld, g.c_bs, g.scale,
                       reinterpret_cast<float*>(g.c), g.c_ld, g.stream_f16, g.stream_guard);
}
NATINF_SG_HIDDEN void launch_patch_embed(const float* z, const float* Wt, const float* bias, const float* pos, float* x, int C, int g, int D, int64_t rows, int x_f16, uint32_t* guard,
                                         void* stream) {
    const dim3 grid((unsigned)((D + 255) / 256), (unsigned)((rows + PE_TOK - 1) / PE_TOK));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (x_f16) hipLaunchKernelGGL(k_patch_embed_guard<true>, grid, dim3(256), 0, s, z, Wt, bias, pos, x, C, g, D, rows, guard);
    else hipLaunchKernelGGL(k_patch_embed_guard<false>, grid, dim3(256), 0, s, z, Wt, bias, pos, x, C, g, D, rows, guard);
}
}  // namespace ncsn_sg
