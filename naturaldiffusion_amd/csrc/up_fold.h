// up_fold.h -- Conv_0 of the 16 -> 32 up-sampling res-block as four 2x2 phase convolutions (natinf_set_fuse_up_fold): the weight fold and the launch's kernel.
//
// Reference arithmetic: ResnetBlockBigGANpp(up=True), layerspp.py:242-274: h = Conv_0(naive_upsample_2d(act(GroupNorm_0(x)))).  A 3x3 convolution over a 2x
// nearest-up-sampled image is exactly four 2x2 convolutions over the low-resolution image, one per output parity (a, b): 4 taps per output pixel instead of 9.
// The K loop and the epilogue are gemm_dma.h's (gemm_dma_tile / packed_tile_epilogue with UPW); included by up_fold.hip only.
#pragma once
#include "gemm_dma.h"

namespace ncsn {

// Conv_0 of an up-sampling res-block: conv3x3(nearest_up_2x(h)) is four 2x2 convolutions over h itself, one per output parity (a, b) (k_conv_gn_upfold below): output pixel
// (2 i + a, 2 j + b) reads rows i + a - 1 + ty and columns j + b - 1 + tx of h.  src [N][Cin][3][3] (fp32) -> the phase kernels Wp[a][b][ty][tx], summed in fp32 in a FIXED
// order -- rows first, then columns, each pair as (W[lo] + W[hi]):
//   rows     a = 0: R[0][kx] = W[0][kx],            R[1][kx] = W[1][kx] + W[2][kx];        a = 1: R[0][kx] = W[0][kx] + W[1][kx],  R[1][kx] = W[2][kx]
//   columns  b = 0: Wp[ty][0] = R[ty][0],           Wp[ty][1] = R[ty][1] + R[ty][2];       b = 1: Wp[ty][0] = R[ty][0] + R[ty][1], Wp[ty][1] = R[ty][2]
// then times wmul and ONE rounding to bf16 (never less precise than rounding the nine taps: |x| eps |W0 + W1| <= |x| eps (|W0| + |W1|)).
// dst (may be null): bf16 [4 N][4 Cin], phase-major (row (2 a + b) * N + n), K order ((c / 64) * 4 + 2 ty + tx) * 64 + c % 64 (Cin % 64 == 0);
// dst32 (may be null; tests): the values before the rounding, fp32 [2][2][N][Cin][2][2] = [a][b][n][c][ty][tx].  One thread per (n, c): no fp32 temporary in memory.
__global__ void k_fold_up_conv(const float* __restrict__ src, bf16* __restrict__ dst, float* __restrict__ dst32, int N, int Cin, float wmul)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * Cin) return;
    const int c = (int)(i % Cin), n = (int)(i / Cin);
    float w[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) w[t] = src[i * 9 + t];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        float R[2][3];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            R[0][kx] = a == 0 ? w[kx] : w[kx] + w[3 + kx];
            R[1][kx] = a == 0 ? w[3 + kx] + w[6 + kx] : w[6 + kx];
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int ty = 0; ty < 2; ++ty)
#pragma unroll
                for (int tx = 0; tx < 2; ++tx) {
                    const float f = b == 0 ? (tx == 0 ? R[ty][0] : R[ty][1] + R[ty][2]) : (tx == 0 ? R[ty][0] + R[ty][1] : R[ty][2]);
                    const float v = f * wmul;
                    const int ph = 2 * a + b;
                    if (dst) dst[((int64_t)ph * N + n) * (4 * Cin) + ((c >> 6) * 4 + 2 * ty + tx) * 64 + (c & 63)] = (bf16)v;
                    if (dst32) dst32[(((int64_t)ph * N + n) * Cin + c) * 4 + 2 * ty + tx] = v;
                }
    }
}

// the up-fold launch: the hand-pipelined 256 x 256 tile (one 16x16 input image x one phase of 256 output channels), LDS-DMA issued by one wave per SIMD
template <int EPI>
__global__ __launch_bounds__(512, 2) void k_conv_gn_upfold(const GemmArgs g) { gemm_dma_tile<2, 4, 8, 4, 6, EPI, 16>(g); }
using UpFoldCfg = DmaCfg<2, 4, 8, 4>;

}  // namespace ncsn
