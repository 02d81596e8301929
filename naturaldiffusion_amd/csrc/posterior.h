// posterior.h -- kernels of the posterior statistics (include/natinf_posterior.h), included by posterior.hip only.
//
//   k_post_norms   |f_j|^2 per row in fp64 (the square of a bf16 value is exact in fp32)
//   k_post_dots    C[i][j] = sum_k (hi + mid + lo)[i][k] * f[j][k] on v_mfma_f32_32x32x16_bf16, split over K into fp64 partial sums
//   k_post_rows    per row i: the fp64 softmax over j of (2 C_ij - |f_j|^2) / (2 sigma^2), reduced to p_ii and max_j p_ij
//   k_post_planes  hi + mid + lo as fp32 (test hook)
//
// k_post_samples, which writes the planes, lives in ni_step.hip: it shares philox_normals with natinf_randn_philox_f32 and that unit's
// -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "posterior_ws.h"

namespace post {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int THREADS = 256;
constexpr int LDS_ROW = BK + 8;                 // bf16 per LDS row: 144 bytes, so the 16 rows one ds_read_b128 phase touches start 36 banks apart -- no conflict
constexpr int A_CHUNKS = 3 * BM * BK / 8 / THREADS;     // 16-byte chunks per thread and K tile: 6 of the three planes
constexpr int B_CHUNKS = BN * BK / 8 / THREADS;         // 4 of f

// fixed-tree block reduction over 256 threads (deterministic: the same bits on every run); every thread returns the result
template <bool kMax>
__device__ __forceinline__ double block_reduce(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = kMax ? fmax(red[t], red[t + s]) : red[t] + red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// one block per row j: 16-byte loads, squares in fp32 (exact), sum in fp64
__global__ __launch_bounds__(THREADS) void k_post_norms(const bf16x8* __restrict__ f, double* __restrict__ norms, int d8)
{
    __shared__ double red[THREADS];
    const bf16x8* row = f + (int64_t)blockIdx.x * d8;
    double acc = 0.0;
    for (int c = threadIdx.x; c < d8; c += THREADS) {
        const bf16x8 v = row[c];
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float x = (float)v[e]; acc += (double)(x * x); }
    }
    acc = block_reduce<false>(acc, red);
    if (threadIdx.x == 0) norms[blockIdx.x] = acc;
}

// Block (bx, by, bz): rows i0 = 64 by .. of s against rows j0 = 128 bx .. of f over K tiles [bz T / S, (bz + 1) T / S).  Four waves, wave w owns the
// 32 x 64 piece at (32 (w & 1), 64 (w >> 1)): two 32x32 accumulators, each fed by the three planes against the same f fragment.  Operands go
// global -> registers -> LDS (the next tile's loads are in flight during the MFMAs); rows past n are zeros, never read.  Every product
// bf16 x bf16 is exact in fp32; the fp32 accumulators are added into fp64 ones after FLUSH_TILES tiles, and the fp64 sums are the partial.
__global__ __launch_bounds__(THREADS, 2) void k_post_dots(
    const __bf16* __restrict__ planes, const __bf16* __restrict__ f, double* __restrict__ partial, int n, int d, int splits)
{
    __shared__ __attribute__((aligned(16))) __bf16 sA[3 * BM * LDS_ROW];
    __shared__ __attribute__((aligned(16))) __bf16 sB[BN * LDS_ROW];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int i0 = blockIdx.y * BM, j0 = blockIdx.x * BN;
    const int ktiles = d / BK;
    const int kt0 = (int)((int64_t)blockIdx.z * ktiles / splits), kt1 = (int)((int64_t)(blockIdx.z + 1) * ktiles / splits);

    // this thread's chunks of a K tile: chunk c = t + 256 u is (row c >> 3, 16-byte column c & 7) of the stacked [3 * 64] (A) or [128] (B) rows
    const __bf16* ga[A_CHUNKS];
    const __bf16* gb[B_CHUNKS];
    bool oka[A_CHUNKS], okb[B_CHUNKS];
    int la[A_CHUNKS], lb[B_CHUNKS];
#pragma unroll
    for (int u = 0; u < A_CHUNKS; ++u) {
        const int c = t + THREADS * u, srow = c >> 3, col = (c & 7) * 8, plane = srow / BM, row = srow - plane * BM;
        oka[u] = i0 + row < n;
        ga[u] = planes + ((int64_t)plane * n + (oka[u] ? i0 + row : 0)) * d + col;
        la[u] = srow * LDS_ROW + col;
    }
#pragma unroll
    for (int u = 0; u < B_CHUNKS; ++u) {
        const int c = t + THREADS * u, row = c >> 3, col = (c & 7) * 8;
        okb[u] = j0 + row < n;
        gb[u] = f + (int64_t)(okb[u] ? j0 + row : 0) * d + col;
        lb[u] = row * LDS_ROW + col;
    }
    bf16x8 ra[A_CHUNKS], rb[B_CHUNKS];
    const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    auto fetch = [&](int kt) __attribute__((always_inline)) {
        const int k = kt * BK;
#pragma unroll
        for (int u = 0; u < A_CHUNKS; ++u) ra[u] = oka[u] ? *reinterpret_cast<const bf16x8*>(ga[u] + k) : zero;
#pragma unroll
        for (int u = 0; u < B_CHUNKS; ++u) rb[u] = okb[u] ? *reinterpret_cast<const bf16x8*>(gb[u] + k) : zero;
    };

    // MFMA operand maps: lane l holds A[row l & 31][k = 8 (l >> 5) + e] and B[k = 8 (l >> 5) + e][col l & 31], e = 0..7
    const int fr = lane & 31, fk = (lane >> 5) * 8;
    const __bf16* pa = sA + ((w & 1) * 32 + fr) * LDS_ROW + fk;
    const __bf16* pb = sB + ((w >> 1) * 64 + fr) * LDS_ROW + fk;

    f32x16 acc[2];
    double sum[2][16];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[q][r] = 0.0f; sum[q][r] = 0.0; }

    fetch(kt0);
    for (int kt = kt0; kt < kt1; ++kt) {
        __syncthreads();                                    // the previous tile's fragment reads are done
#pragma unroll
        for (int u = 0; u < A_CHUNKS; ++u) *reinterpret_cast<bf16x8*>(sA + la[u]) = ra[u];
#pragma unroll
        for (int u = 0; u < B_CHUNKS; ++u) *reinterpret_cast<bf16x8*>(sB + lb[u]) = rb[u];
        __syncthreads();
        if (kt + 1 < kt1) fetch(kt + 1);
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(pb + ks * 16);
            const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(pb + 32 * LDS_ROW + ks * 16);
#pragma unroll
            for (int p = 2; p >= 0; --p) {                  // lo, mid, hi: the small terms first
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(pa + p * BM * LDS_ROW + ks * 16);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b1, acc[1], 0, 0, 0);
            }
        }
        if ((kt - kt0 + 1) % FLUSH_TILES == 0 || kt + 1 == kt1) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) { sum[q][r] += (double)acc[q][r]; acc[q][r] = 0.0f; }
        }
    }

    // C/D map: register r of lane l is (row (r & 3) + 8 (r >> 2) + 4 (l >> 5), col l & 31): 32 consecutive doubles per store
    double* out = partial + (int64_t)blockIdx.z * n * n;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int j = j0 + (w >> 1) * 64 + q * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + (w & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (i < n && j < n) out[(int64_t)i * n + j] = sum[q][r];
        }
    }
}

// One block per row i.  raw_j = 2 C_ij - |f_j|^2 with C_ij the fp64 sum of the partials in split order; m = max_j raw_j;
// S = sum_j exp((raw_j - m) * inv2s2).  The difference is taken BEFORE the scaling, so the maximum's term is exp(0) = 1 exactly for any
// sigma, every term is in [0, 1] and S >= 1: p_max = 1 / S and p_diag = exp((raw_i - m) * inv2s2) / S are finite, in [0, 1], p_diag <= p_max.
__global__ __launch_bounds__(THREADS) void k_post_rows(
    const double* __restrict__ partial, const double* __restrict__ norms, int n, int splits, double inv2s2,
    double* __restrict__ p_diag, double* __restrict__ p_max)
{
    __shared__ double red[THREADS];
    __shared__ double diag;
    const int i = blockIdx.x;
    const double* row = partial + (int64_t)i * n;
    const int64_t nn = (int64_t)n * n;
    auto raw = [&](int j) __attribute__((always_inline)) {
        double c = 0.0;
        for (int s = 0; s < splits; ++s) c += row[s * nn + j];
        return 2.0 * c - norms[j];
    };
    double m = -INFINITY;
    for (int j = threadIdx.x; j < n; j += THREADS) m = fmax(m, raw(j));
    m = block_reduce<true>(m, red);
    double sum = 0.0;
    for (int j = threadIdx.x; j < n; j += THREADS) {
        const double dlt = raw(j) - m;
        const double e = dlt < 0.0 ? exp(dlt * inv2s2) : 1.0;
        sum += e;
        if (j == i) diag = e;
    }
    sum = block_reduce<false>(sum, red);                    // its barriers also publish `diag`
    if (threadIdx.x == 0) { p_diag[i] = diag / sum; p_max[i] = 1.0 / sum; }
}

// test hook: s = (hi + mid) + lo, both sums exact in fp32
__global__ __launch_bounds__(THREADS) void k_post_planes(const bf16x8* __restrict__ planes, float4* __restrict__ s_out, int64_t nvec)
{
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (v < nvec) {
        const bf16x8 hi = planes[v], mid = planes[nvec + v], lo = planes[2 * nvec + v];
        float s[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = ((float)hi[e] + (float)mid[e]) + (float)lo[e];
        s_out[2 * v] = make_float4(s[0], s[1], s[2], s[3]);
        s_out[2 * v + 1] = make_float4(s[4], s[5], s[6], s[7]);
    }
}

}  // namespace post
