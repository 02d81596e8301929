// ideal.h -- kernels of the ideal denoiser, the posterior mean over a training set (include/natinf_ideal.h), included by prdc.hip
// behind prdc.h, whose sweep they are built around.
//
//   k_ideal_tplanes  planes [3][N][d] -> transposed planes [3][d][Np], Np = ceil(N / 64) * 64, pad columns zero (once per training set)
//   (k_prdc_dist2    prdc.h's own kernel stages the d2 chunk [rows][N], launched from an entry without the test hook's size cap)
//   k_ideal_rows     per staged row: m, lse, pmax, nearest and the weights w = fp32(exp(z - lse)) as three bf16 planes [3][R][Np]
//   k_ideal_part     sweep<PART>: W . F over one range of PART_K columns j per block, rows = the weight planes, columns = the transposed planes, K = Np;
//                    fp64 partials [ranges][rows][d]
//   k_ideal_merge    the ranges' partials added in ascending range order; x0 = fp32(mean) and, when asked, out = fp32((x - alpha mean) / sigma)
//   k_ideal_wdebug   hi + mid + lo of the weight planes as fp32 (test hook)
//
// Every output of a row is a function of that row, its scalars and the training set: d2_ij is (prdc.h); the row stage sees one row; a range's partial is a
// function of the two operand rows and the range; the ranges are cut at multiples of PART_K whatever the call looks like, and merged in ascending order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace ideal {

using prdc::bf16x8;
constexpr int TP = 64;                  // the transpose's tile: 64 rows x 64 values, bf16
constexpr int TP_ROW = TP + 8;          // bf16 per LDS row: 144 bytes, a multiple of 16

// grid (Np / 64, d / 64, 3): tile (n0 = 64 bx, e0 = 64 by) of plane bz through LDS, 16-byte accesses on both sides; rows past n are zeros
__global__ __launch_bounds__(prdc::THREADS) void k_ideal_tplanes(const __bf16* __restrict__ planes, int64_t n, int d, int64_t np, __bf16* __restrict__ tplanes)
{
    __shared__ __attribute__((aligned(16))) __bf16 s[TP * TP_ROW];
    const int t = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * TP;
    const int e0 = blockIdx.y * TP;
    const __bf16* src = planes + (int64_t)blockIdx.z * n * d;
    __bf16* dst = tplanes + (int64_t)blockIdx.z * d * np;
    const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int c = t + prdc::THREADS * u, r = c >> 3, cc = (c & 7) * 8;
        *reinterpret_cast<bf16x8*>(s + r * TP_ROW + cc) = n0 + r < n ? *reinterpret_cast<const bf16x8*>(src + (n0 + r) * d + e0 + cc) : zero;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int c = t + prdc::THREADS * u, e = c >> 3, nn = (c & 7) * 8;
        bf16x8 v;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = s[(nn + k) * TP_ROW + e];
        *reinterpret_cast<bf16x8*>(dst + (int64_t)(e0 + e) * np + n0 + nn) = v;
    }
}

// grid (column tiles of d, row blocks, K ranges): partial [ranges][n_rows][n_cols]
__global__ __launch_bounds__(prdc::THREADS, 2) void k_ideal_part(prdc::Operands op, double* __restrict__ partial)
{
    prdc::sweep<prdc::PART>(op, 1, partial, nullptr, nullptr, nullptr, nullptr);
}

__device__ __forceinline__ double logit(double c, double d2) { return d2 == INFINITY ? -INFINITY : -(c * d2); }

// One wave per row of the weight planes [3][plane_rows][np]; block i >= n_rows only writes its row of zeros.  Row i of the staged d2 [n_rows][n_cols] is read
// three times (400 KB at 50,000 columns): lane l takes the columns l, l + 64, ... in ascending order for the largest logit, the nearest column and the sum of
// exp(z - m) -- k_is_rows' 64 strided partial sums and wave_sum's tree --, then eight columns in a row for the weights, which no sum crosses.  The nearest
// column is chosen on d2 in pair_less's order (c = 0 makes every logit equal).  w = fp32(p) splits as k_prdc_planes splits a feature; pad columns are zeros.
__global__ __launch_bounds__(64) void k_ideal_rows(const double* __restrict__ d2, int n_rows, int n_cols, int64_t np, const double* __restrict__ c,
                                                   __bf16* __restrict__ planes, int64_t plane_elems, double* __restrict__ lse_out,
                                                   double* __restrict__ pmax_out, int* __restrict__ nearest_out)
{
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    __bf16* wr = planes + i * np;
    if (i >= n_rows) {
        const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int64_t j0 = lane * 8; j0 < np; j0 += 512)
#pragma unroll
            for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x8*>(wr + p * plane_elems + j0) = zero;
        return;
    }
    const double* dr = d2 + i * n_cols;
    const double ci = c[i];
    double m = -INFINITY, best = INFINITY;
    int bj = -1;
#pragma unroll 4
    for (int j = lane; j < n_cols; j += 64) {
        const double v = dr[j];
        m = fmax(m, logit(ci, v));
        const bool less = v < best;                             // a lane meets its columns in ascending order: the first of equal distances stays
        best = less ? v : best;
        bj = less ? j : bj;
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        m = fmax(m, __shfl_xor(m, s));
        const double ob = __shfl_xor(best, s);
        const int oj = __shfl_xor(bj, s);
        const bool less = oj >= 0 && (bj < 0 || prdc::pair_less(ob, oj, best, bj));
        best = less ? ob : best;
        bj = less ? oj : bj;
    }
    double se = 0.0;
#pragma unroll 4
    for (int j = lane; j < n_cols; j += 64) se += exp(logit(ci, dr[j]) - m);
    se = prdc::wave_sum(se);
    const double lse = m + log(se);
    for (int64_t j0 = lane * 8; j0 < np; j0 += 512) {
        bf16x8 hi, mid, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t j = j0 + e;
            const float w = j < n_cols ? (float)exp(logit(ci, dr[j]) - lse) : 0.0f;
            hi[e] = (__bf16)w;
            const float r1 = w - (float)hi[e];
            mid[e] = (__bf16)r1;
            const float r2 = r1 - (float)mid[e];
            lo[e] = (__bf16)r2;
        }
        *reinterpret_cast<bf16x8*>(wr + j0) = hi;
        *reinterpret_cast<bf16x8*>(wr + plane_elems + j0) = mid;
        *reinterpret_cast<bf16x8*>(wr + 2 * plane_elems + j0) = lo;
    }
    if (lane == 0) {
        if (lse_out) lse_out[i] = lse;
        if (pmax_out) pmax_out[i] = exp(m - lse);
        if (nearest_out) nearest_out[i] = bj;
    }
}

// one thread per (row, value): the ranges' partials in ascending range order, then the finishing arithmetic, every operation rounded once (no contraction)
__global__ __launch_bounds__(prdc::THREADS) void k_ideal_merge(const double* __restrict__ partial, int64_t n_rows, int d, int ranges, const float* __restrict__ x,
                                                               const double* __restrict__ alpha, const double* __restrict__ sigma, float* __restrict__ x0_out,
                                                               float* __restrict__ out)
{
    const int64_t v = (int64_t)blockIdx.x * prdc::THREADS + threadIdx.x, slab = n_rows * d;
    if (v >= slab) return;
    double mean = partial[v];
    for (int r = 1; r < ranges; ++r) mean += partial[r * slab + v];
    x0_out[v] = (float)mean;
    if (out) {
        const int64_t i = v / d;
        out[v] = (float)__ddiv_rn(__dsub_rn((double)x[v], __dmul_rn(alpha[i], mean)), sigma[i]);
    }
}

// one thread per (row, column): (hi + mid) + lo, both sums exact in fp32
__global__ __launch_bounds__(prdc::THREADS) void k_ideal_wdebug(const __bf16* __restrict__ planes, int64_t plane_elems, int64_t n_rows, int n_cols, int64_t np,
                                                                float* __restrict__ w_out)
{
    const int64_t v = (int64_t)blockIdx.x * prdc::THREADS + threadIdx.x;
    if (v >= n_rows * n_cols) return;
    const int64_t o = v / n_cols * np + v % n_cols;
    w_out[v] = ((float)planes[o] + (float)planes[plane_elems + o]) + (float)planes[2 * plane_elems + o];
}

}  // namespace ideal
