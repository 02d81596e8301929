// prdc.h -- kernels of the k-nearest-neighbour manifold metrics (include/natinf_prdc.h), included by prdc.hip only.
//
//   k_prdc_planes  fp32 features -> three bf16 planes hi + mid + lo == x (every residual exact in fp32) and |x_i|^2 in fp64
//   k_prdc_knn     per row i the K_MAX smallest d2_ij over a range of column tiles, as a sorted list that stays in registers
//   k_prdc_merge   the lists of the column splits -> the k-th smallest per row
//   k_nn_nearest   k_prdc_knn with the column index carried through the list: per row the K_MAX smallest pairs (d2_ij, j) (include/natinf_nn.h)
//   k_nn_merge     the pair lists of the column splits -> the k smallest pairs per row
//   k_prdc_balls   per row i the counts #{j: d2_ij <= r2_cols[j]} and #{j: d2_ij <= r2_rows[i]}
//   k_prdc_dist2   the same tiles written out (test hook)
//   k_kid_sums     per row i the fp64 sum of (gamma a_i.b_j + coef0)^3 over a range of column tiles (include/natinf_kid.h)
//   k_kid_merge    the partial sums of the column splits, added in ascending split order
//   k_is_logits    the same tiles as z_ij = a_i.w_j + bias_j, written to a staging buffer (include/natinf_is.h)
//   k_is_rows      per staged row its log-sum-exp, negative entropy and first largest class, and the rows' fixed-point class probabilities added per class
//   (ideal.h, included behind this file, builds the ideal denoiser on the sweep: its weighted sum is sweep<PART>; include/natinf_ideal.h)
//
// d2_ij = max(0, (|a_i|^2 + |b_j|^2) - 2 a_i.b_j) in fp64.  a_i.b_j is six bf16 MFMA passes (lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi: the small
// terms first; the three dropped products are below 2^-26 of |a_k b_k|) whose products are all exact in the fp32 accumulator; the accumulator is added
// into an fp64 one after FLUSH_TILES K tiles.  The k order of one (i, j) is the same in every tile of every kernel here, so d2_ij is a function of the two
// rows only: not of the tile it falls into, the row block, the column split or the call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace prdc {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int THREADS = 256;
constexpr int BM = 64;                  // rows (i) per block
constexpr int BN = 128;                 // columns (j) per tile
constexpr int BK = 32;                  // values of k per LDS tile
// The fp32 accumulators are added into the fp64 ones after 2 tiles = 64 values of k.  Every MFMA rounds the running sum to fp32, so the error grows with the
// sum's size: flushed after 512 values (k_post_dots' interval) these distances measured 2^-21.1 of |a|^2 + |b|^2 at d = 192 and 2^-21.4 at d = 2048, a little
// worse than torch's fp32 statement; the error falls with the number of flushes.
// -DNATINF_PRDC_FLUSH_TILES=16 (make EXTRA=..., with BUILD and OUT outside the package) builds the 512-value interval those figures were taken with.
#ifndef NATINF_PRDC_FLUSH_TILES
#define NATINF_PRDC_FLUSH_TILES 2
#endif
constexpr int FLUSH_TILES = NATINF_PRDC_FLUSH_TILES;
static_assert(FLUSH_TILES >= 1 && FLUSH_TILES <= 16, "at most 512 values of k between two flushes");
constexpr int K_MAX = 8;                // length of the sorted list
constexpr int LDS_ROW = BK + 8;         // bf16 per LDS row: 80 bytes, the 16 rows of one ds_read_b128 phase start 20 banks apart -- 16 distinct 4-bank groups
constexpr int A_CHUNKS = 3 * BM * BK / 8 / THREADS;     // 16-byte chunks per thread and K tile: 3 (one per plane)
constexpr int B_CHUNKS = 3 * BN * BK / 8 / THREADS;     // 6
constexpr int STAGE_COLS = BN / 2;      // one of a wave's two accumulators at a time goes through LDS: 64 x 64 doubles
constexpr int STAGE_ROW = STAGE_COLS + 1;
constexpr int OPERAND_BYTES = 3 * (BM + BN) * LDS_ROW * 2;
constexpr int STAGE_BYTES = BM * STAGE_ROW * 8;
constexpr int LDS_BYTES = OPERAND_BYTES > STAGE_BYTES ? OPERAND_BYTES : STAGE_BYTES;

enum Mode { KNN = 0, BALLS = 1, DIST = 2, KSUM = 3, LOGIT = 4, NN = 5, PART = 6 };
constexpr int PART_K = NATINF_IDEAL_K_RANGE;        // PART: values of k per block (include/natinf_ideal.h)
static_assert(PART_K >= 64 && PART_K % (BK * FLUSH_TILES) == 0 && PART_K % 64 == 0, "a K range is whole flush intervals of 64 values");

struct Operands {
    const __bf16* a;        // [3][n_rows][d], plane p at a + p * a_plane
    const double* na;       // [n_rows] (KSUM, LOGIT, PART: not read)
    const __bf16* b;        // [3][n_cols][d], plane p at b + p * b_plane
    const double* nb;       // [n_cols] (KSUM, LOGIT, PART: not read)
    int64_t a_plane, b_plane;   // elements between two planes: n * d for a whole set, the whole set's for a row range taken in place
    int n_rows, n_cols, d;
    int64_t self_offset;    // column self_offset + i is left out of row i; -1: none
};

// fixed-tree block reduction over 256 threads (the same bits on every run); thread 0's return value is the sum
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// one block per row: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), both differences exact in fp32; the norm from the fp32 values
__global__ __launch_bounds__(THREADS) void k_prdc_planes(const float4* __restrict__ x, bf16x8* __restrict__ planes, double* __restrict__ norms,
                                                         int d8, int64_t plane_vecs)
{
    __shared__ double red[THREADS];
    const int64_t row = blockIdx.x;
    double acc = 0.0;
    for (int c = threadIdx.x; c < d8; c += THREADS) {
        const int64_t v = row * d8 + c;
        const float4 x0 = x[2 * v], x1 = x[2 * v + 1];
        const float s[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        bf16x8 hi, mid, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            hi[e] = (__bf16)s[e];
            const float r1 = s[e] - (float)hi[e];
            mid[e] = (__bf16)r1;
            const float r2 = r1 - (float)mid[e];
            lo[e] = (__bf16)r2;
            acc += (double)s[e] * (double)s[e];
        }
        planes[v] = hi;
        planes[plane_vecs + v] = mid;
        planes[2 * plane_vecs + v] = lo;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) norms[row] = acc;
}

// sorted insert into an ascending list held in registers (every index is a compile-time constant)
__device__ __forceinline__ void list_insert(double (&L)[K_MAX], double v) {
    if (v < L[K_MAX - 1]) {
#pragma unroll
        for (int s = K_MAX - 1; s > 0; --s) L[s] = v < L[s - 1] ? L[s - 1] : (v < L[s] ? v : L[s]);
        L[0] = v < L[0] ? v : L[0];
    }
}

// (d2, column) pairs in lexicographic order: among equal distances the lower column comes first.  An empty slot is (+inf, -1): nothing is below it but a finite
// distance, so a column at +inf never enters a list (a NaN never gets here: the max(0, .) of d2 turns it into 0).
__device__ __forceinline__ bool pair_less(double v, int j, double w, int i) { return v < w || (v == w && j < i); }

// list_insert for pairs: the lists the callers merge hold disjoint columns, so no pair is ever met twice
__device__ __forceinline__ void pair_insert(double (&L)[K_MAX], int (&I)[K_MAX], double v, int j) {
    if (pair_less(v, j, L[K_MAX - 1], I[K_MAX - 1])) {
#pragma unroll
        for (int s = K_MAX - 1; s > 0; --s) {
            const bool up = pair_less(v, j, L[s - 1], I[s - 1]), here = pair_less(v, j, L[s], I[s]);
            L[s] = up ? L[s - 1] : (here ? v : L[s]);
            I[s] = up ? I[s - 1] : (here ? j : I[s]);
        }
        const bool here = pair_less(v, j, L[0], I[0]);
        L[0] = here ? v : L[0];
        I[0] = here ? j : I[0];
    }
}

// Block (bx, by): rows i0 = 64 by .. of A against the column tiles [bx T / S, (bx + 1) T / S) of B, T = ceil(n_cols / 128) (DIST: the one tile bx).  The column
// split is the fast grid index: blocks that follow each other share their rows of A, and with S a multiple of 8 one XCD sweeps one column range.  Four waves,
// wave w owns the 32 x 64 piece at (32 (w & 1), 64 (w >> 1)) of a tile: two 32x32 accumulators.  Operands go global -> registers -> LDS, the next K tile's
// loads (across the column tile's end too) in flight during the MFMAs; rows and columns past n are zeros, never read.  After a column tile's last K tile the
// fp64 d2 values go through LDS, one accumulator at a time, to the thread that owns (row t >> 2, every fourth column from t & 3): it keeps a sorted list
// (KNN) or two counters (BALLS) over the whole sweep.  Columns past n_cols and the left-out column never reach a list or a counter.
// KSUM stages nothing per tile: the lane that holds s_ij forms k = (gamma s + coef0)^3 in fp64 and adds it to the running sum of its row and column class
// (one of 32 columns mod 32 of the wave's half tile), the tile's two accumulators and then the tiles in ascending order; after the sweep the 64 class sums of
// a row go through LDS once and are added in a fixed order.  The order depends on the column range of the block alone, never on where the row sits in it.
// LOGIT is DIST without the norms: the lane that holds s_ij writes z_ij = s_ij + bias[j] to row i of a staging buffer whose rows are whole tiles long
// (ceil(n_cols / 128) * 128 doubles); columns past n_cols are not written.
// PART is LOGIT over one range of k: block (bx, by, bz) forms the dot products of the one tile bx over k in [PART_K bz, min(PART_K (bz + 1), d)) and writes them,
// without a bias, to slab bz of a buffer [ranges][n_rows][n_cols] (csrc/ideal.h).  PART_K is whole flush intervals, so the fp32 accumulator is flushed at the
// same k as in an unsplit sweep, and a range's value is a function of the two rows and the range only.
// NN is KNN with the column beside every distance: the same staged values reach the same threads, which keep (d2, j) pairs in pair_less's order.  A thread
// does not meet its columns in ascending order (a tile's two accumulators interleave), so the tie rule is in the comparison, not in the order of arrival.
template <int MODE>
__device__ __forceinline__ void sweep(const Operands& op, int splits, double* __restrict__ out_f64, const double* __restrict__ r2_rows,
                                      const double* __restrict__ r2_cols, int* __restrict__ cnt_row_ball, int* __restrict__ cnt_col_ball,
                                      double gamma = 0.0, double coef0 = 0.0, const float* __restrict__ bias = nullptr, int* __restrict__ out_idx = nullptr)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];
    __shared__ double sNa[BM], sNb[BN], sR2c[BN];
    __bf16* sA = reinterpret_cast<__bf16*>(smem);
    __bf16* sB = sA + 3 * BM * LDS_ROW;
    double* sD = reinterpret_cast<double*>(smem);

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int i0 = blockIdx.y * BM;
    const int kbase = MODE == PART ? (int)blockIdx.z * PART_K : 0;
    const int ktiles = MODE == PART ? (op.d - kbase < PART_K ? op.d - kbase : PART_K) / BK : op.d / BK;
    const int ctiles = (op.n_cols + BN - 1) / BN;
    const int ct0 = (MODE == DIST || MODE == LOGIT || MODE == PART) ? (int)blockIdx.x : (int)((int64_t)blockIdx.x * ctiles / splits);
    const int ct1 = (MODE == DIST || MODE == LOGIT || MODE == PART) ? ct0 + 1 : (int)((int64_t)(blockIdx.x + 1) * ctiles / splits);
    const int64_t d = op.d;

    // this thread's chunks of a K tile: chunk c = t + 256 u is (row c >> 2, 16-byte column c & 3) of the stacked [3 * 64] (A) or [3 * 128] (B) rows
    const int crow = t >> 2, ccol = (t & 3) * 8;
    const bool oka = i0 + crow < op.n_rows;
    const __bf16* ga = op.a + (int64_t)(oka ? i0 + crow : 0) * d + ccol;
    const int64_t a_plane = op.a_plane, b_plane = op.b_plane;
    bf16x8 ra[A_CHUNKS], rb[B_CHUNKS];
    const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    int f_ct = ct0, f_kt = 0;                                // the tile the next fetch loads
    auto fetch = [&]() __attribute__((always_inline)) {
        const int k = kbase + f_kt * BK;
#pragma unroll
        for (int u = 0; u < A_CHUNKS; ++u) ra[u] = oka ? *reinterpret_cast<const bf16x8*>(ga + u * a_plane + k) : zero;
#pragma unroll
        for (int u = 0; u < B_CHUNKS; ++u) {
            const int64_t j = (int64_t)f_ct * BN + crow + 64 * (u & 1);
            rb[u] = j < op.n_cols ? *reinterpret_cast<const bf16x8*>(op.b + (u >> 1) * b_plane + j * d + ccol + k) : zero;
        }
        if (++f_kt == ktiles) { f_kt = 0; ++f_ct; }
    };

    // MFMA operand maps: lane l holds A[row l & 31][k = 8 (l >> 5) + e] and B[k = 8 (l >> 5) + e][col l & 31], e = 0..7
    const int fr = lane & 31, fk = (lane >> 5) * 8;
    const __bf16* pa = sA + ((w & 1) * 32 + fr) * LDS_ROW + fk;
    const __bf16* pb = sB + ((w >> 1) * 64 + fr) * LDS_ROW + fk;

    if (MODE != KSUM && MODE != LOGIT && MODE != PART && t < BM) sNa[t] = i0 + t < op.n_rows ? op.na[i0 + t] : 0.0;      // published by the first barrier below

    f32x16 acc[2];
    double sum[2][16];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[q][r] = 0.0f; sum[q][r] = 0.0; }

    // the scanning thread's row and its state over the sweep
    const int srow = t >> 2, sc0 = t & 3;
    const int64_t si = (int64_t)i0 + srow;
    double L[K_MAX];
#pragma unroll
    for (int s = 0; s < K_MAX; ++s) L[s] = INFINITY;
    int LI[K_MAX];                                              // NN: the column of L[s]
#pragma unroll
    for (int s = 0; s < K_MAX; ++s) LI[s] = -1;
    int n_rowball = 0, n_colball = 0;
    double my_r2 = 0.0;
    if (MODE == BALLS) my_r2 = (r2_rows && si < op.n_rows) ? r2_rows[si] : -INFINITY;
    const int64_t skip = op.self_offset >= 0 ? op.self_offset + si : -1;
    double rsum[16];                                            // KSUM: register r's row, this lane's column class
#pragma unroll
    for (int r = 0; r < 16; ++r) rsum[r] = 0.0;

    if (ct0 < ct1) fetch();
    for (int ct = ct0; ct < ct1; ++ct) {
        for (int kt = 0; kt < ktiles; ++kt) {
            __syncthreads();                                    // the previous tile's fragment reads (or the scan of the staged d2) are done
#pragma unroll
            for (int u = 0; u < A_CHUNKS; ++u) *reinterpret_cast<bf16x8*>(sA + (u * BM + crow) * LDS_ROW + ccol) = ra[u];
#pragma unroll
            for (int u = 0; u < B_CHUNKS; ++u) *reinterpret_cast<bf16x8*>(sB + ((u >> 1) * BN + crow + 64 * (u & 1)) * LDS_ROW + ccol) = rb[u];
            __syncthreads();
            if (kt + 1 < ktiles || ct + 1 < ct1) fetch();
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                bf16x8 a[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) a[p] = *reinterpret_cast<const bf16x8*>(pa + p * BM * LDS_ROW + ks * 16);
#pragma unroll
                for (int q = 0; q < 2; ++q) {                   // planes 0 / 1 / 2 = hi / mid / lo: the small products first
                    bf16x8 b[3];
#pragma unroll
                    for (int p = 0; p < 3; ++p) b[p] = *reinterpret_cast<const bf16x8*>(pb + (p * BN + 32 * q) * LDS_ROW + ks * 16);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc[q], 0, 0, 0);
                }
            }
            if ((kt + 1) % FLUSH_TILES == 0 || kt + 1 == ktiles) {
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { sum[q][r] += (double)acc[q][r]; acc[q][r] = 0.0f; }
            }
        }

        // ---- the column tile's epilogue ----
        const int64_t j0 = (int64_t)ct * BN;
        if (MODE == KSUM) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int64_t j = j0 + (w >> 1) * 64 + q * 32 + (lane & 31);
                // the left-out column of register r's row is self_offset + i0 + 32 (w & 1) + 4 (lane >> 5) + (r & 3) + 8 (r >> 2): compare what is left of j
                const int64_t rel = op.self_offset >= 0 ? j - op.self_offset - i0 - (w & 1) * 32 - 4 * (lane >> 5) : -1;
                const bool inside = j < op.n_cols;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const double u = gamma * sum[q][r] + coef0;
                    const double kv = u * u * u;
                    sum[q][r] = 0.0;
                    rsum[r] += (inside && rel != (r & 3) + 8 * (r >> 2)) ? kv : 0.0;
                }
            }
            continue;
        }
        if (MODE == LOGIT) {
            const int64_t ldz = (int64_t)ctiles * BN;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int64_t j = j0 + (w >> 1) * 64 + q * 32 + (lane & 31);
                const bool inside = j < op.n_cols;
                const double bj = (bias && inside) ? (double)bias[j] : 0.0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t i = (int64_t)i0 + (w & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const double z = sum[q][r] + bj;
                    sum[q][r] = 0.0;
                    if (inside && i < op.n_rows) out_f64[i * ldz + j] = z;
                }
            }
            continue;
        }
        if (MODE == PART) {
            double* slab = out_f64 + (int64_t)blockIdx.z * op.n_rows * op.n_cols;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int64_t j = j0 + (w >> 1) * 64 + q * 32 + (lane & 31);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t i = (int64_t)i0 + (w & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (j < op.n_cols && i < op.n_rows) slab[i * op.n_cols + j] = sum[q][r];
                }
            }
            continue;
        }
        if (t < BN) {
            const int64_t j = j0 + t;
            sNb[t] = j < op.n_cols ? op.nb[j] : INFINITY;
            if (MODE == BALLS) sR2c[t] = (r2_cols && j < op.n_cols) ? r2_cols[j] : -INFINITY;
        }
        __syncthreads();                                        // every wave is done with the operands in LDS; the norms are there
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            // C/D map: register r of lane l is (row (r & 3) + 8 (r >> 2) + 4 (l >> 5), col l & 31)
            const int jl = (w >> 1) * 64 + q * 32 + (lane & 31);
            const double nb = sNb[jl];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int il = (w & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const double d2 = fmax(0.0, (sNa[il] + nb) - 2.0 * sum[q][r]);
                sum[q][r] = 0.0;
                if (MODE == DIST) {
                    const int64_t i = (int64_t)i0 + il, j = j0 + jl;
                    if (i < op.n_rows && j < op.n_cols) out_f64[i * op.n_cols + j] = (op.self_offset >= 0 && j == op.self_offset + i) ? INFINITY : d2;
                } else {
                    sD[il * STAGE_ROW + (w >> 1) * 32 + (lane & 31)] = d2;
                }
            }
            if (MODE != DIST) {
                __syncthreads();
#pragma unroll 4
                for (int c = 0; c < STAGE_COLS / 4; ++c) {
                    const int cs = sc0 + 4 * c;                 // staged column cs is column 64 (cs >> 5) + 32 q + (cs & 31) of the tile
                    const int jl2 = (cs >> 5) * 64 + q * 32 + (cs & 31);
                    const int64_t j = j0 + jl2;
                    const double v = sD[srow * STAGE_ROW + cs];
                    if (j < op.n_cols && j != skip) {
                        if (MODE == KNN) list_insert(L, v);
                        if (MODE == NN) pair_insert(L, LI, v, (int)j);
                        if (MODE == BALLS) { n_rowball += v <= my_r2; n_colball += v <= sR2c[jl2]; }
                    }
                }
                __syncthreads();
            }
        }
    }

    if (MODE == KNN) {
        // the four threads of a row hold four lists: after two exchanges every one of them holds the row's K_MAX smallest
#pragma unroll
        for (int step = 1; step <= 2; step <<= 1) {
            double P[K_MAX];
#pragma unroll
            for (int s = 0; s < K_MAX; ++s) P[s] = __shfl_xor(L[s], step);
#pragma unroll
            for (int s = 0; s < K_MAX; ++s) list_insert(L, P[s]);
        }
        if (sc0 == 0 && si < op.n_rows) {
            double* o = out_f64 + ((int64_t)blockIdx.x * op.n_rows + si) * K_MAX;
#pragma unroll
            for (int s = 0; s < K_MAX; ++s) o[s] = L[s];
        }
    }
    if (MODE == NN) {
        // as KNN: the four threads of a row hold the row's four column classes (j mod 4), disjoint at both exchanges
#pragma unroll
        for (int step = 1; step <= 2; step <<= 1) {
            double P[K_MAX];
            int PI[K_MAX];
#pragma unroll
            for (int s = 0; s < K_MAX; ++s) { P[s] = __shfl_xor(L[s], step); PI[s] = __shfl_xor(LI[s], step); }
#pragma unroll
            for (int s = 0; s < K_MAX; ++s) pair_insert(L, LI, P[s], PI[s]);
        }
        if (sc0 == 0 && si < op.n_rows) {
            const int64_t o = ((int64_t)blockIdx.x * op.n_rows + si) * K_MAX;
#pragma unroll
            for (int s = 0; s < K_MAX; ++s) { out_f64[o + s] = L[s]; out_idx[o + s] = LI[s]; }
        }
    }
    if (MODE == KSUM) {
        __syncthreads();                                        // every wave is done with the operands in LDS
#pragma unroll
        for (int r = 0; r < 16; ++r) sD[((w & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * STAGE_ROW + (w >> 1) * 32 + (lane & 31)] = rsum[r];
        __syncthreads();
        double v = 0.0;                                         // thread (row t >> 2, t & 3) adds every fourth class in ascending order, then a two-step tree
#pragma unroll 4
        for (int c = 0; c < STAGE_COLS / 4; ++c) v += sD[srow * STAGE_ROW + sc0 + 4 * c];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        if (sc0 == 0 && si < op.n_rows) out_f64[(int64_t)blockIdx.x * op.n_rows + si] = v;
    }
    if (MODE == BALLS) {
#pragma unroll
        for (int step = 1; step <= 2; step <<= 1) {
            n_rowball += __shfl_xor(n_rowball, step);
            n_colball += __shfl_xor(n_colball, step);
        }
        if (sc0 == 0 && si < op.n_rows) {                       // integer sums: the same total in any order
            if (cnt_row_ball) atomicAdd(cnt_row_ball + si, n_rowball);
            if (cnt_col_ball) atomicAdd(cnt_col_ball + si, n_colball);
        }
    }
}

// lists: [splits][n_rows][K_MAX]
__global__ __launch_bounds__(THREADS, 2) void k_prdc_knn(Operands op, int splits, double* __restrict__ lists)
{
    sweep<KNN>(op, splits, lists, nullptr, nullptr, nullptr, nullptr);
}

// the counters must be zero on entry (the column splits add into them)
__global__ __launch_bounds__(THREADS, 2) void k_prdc_balls(Operands op, int splits, const double* __restrict__ r2_rows, const double* __restrict__ r2_cols,
                                                           int* __restrict__ cnt_row_ball, int* __restrict__ cnt_col_ball)
{
    sweep<BALLS>(op, splits, nullptr, r2_rows, r2_cols, cnt_row_ball, cnt_col_ball);
}

// grid (column tiles, row blocks): d2_out [n_rows][n_cols], the left-out column +inf
__global__ __launch_bounds__(THREADS, 2) void k_prdc_dist2(Operands op, double* __restrict__ d2_out)
{
    sweep<DIST>(op, 1, d2_out, nullptr, nullptr, nullptr, nullptr);
}

// partial: [splits][n_rows], one sum per row and column split
__global__ __launch_bounds__(THREADS, 2) void k_kid_sums(Operands op, int splits, double gamma, double coef0, double* __restrict__ partial)
{
    sweep<KSUM>(op, splits, partial, nullptr, nullptr, nullptr, nullptr, gamma, coef0);
}

// one thread per row: the splits' partial sums in ascending split order
__global__ __launch_bounds__(THREADS) void k_kid_merge(const double* __restrict__ partial, int64_t n_rows, int splits, double* __restrict__ sums_out)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_rows) return;
    double v = partial[i];
    for (int sp = 1; sp < splits; ++sp) v += partial[(int64_t)sp * n_rows + i];
    sums_out[i] = v;
}

// one thread per row: the k-th smallest of the splits' lists (a multiset: equal values count once each)
__global__ __launch_bounds__(THREADS) void k_prdc_merge(const double* __restrict__ lists, int64_t n_rows, int splits, int k, double* __restrict__ r2_out)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_rows) return;
    double L[K_MAX];
#pragma unroll
    for (int s = 0; s < K_MAX; ++s) L[s] = INFINITY;
    for (int sp = 0; sp < splits; ++sp) {
        const double* p = lists + ((int64_t)sp * n_rows + i) * K_MAX;
#pragma unroll
        for (int s = 0; s < K_MAX; ++s) list_insert(L, p[s]);
    }
    double r = L[0];
#pragma unroll
    for (int s = 1; s < K_MAX; ++s) r = s == k - 1 ? L[s] : r;
    r2_out[i] = r;
}

// lists, cols: [splits][n_rows][K_MAX]
__global__ __launch_bounds__(THREADS, 2) void k_nn_nearest(Operands op, int splits, double* __restrict__ lists, int* __restrict__ cols)
{
    sweep<NN>(op, splits, lists, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, nullptr, cols);
}

// one thread per row: the k smallest pairs of the splits' lists (the splits hold disjoint columns) -> d2_out, idx_out [n_rows][k]
__global__ __launch_bounds__(THREADS) void k_nn_merge(const double* __restrict__ lists, const int* __restrict__ cols, int64_t n_rows, int splits, int k,
                                                      double* __restrict__ d2_out, int* __restrict__ idx_out)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_rows) return;
    double L[K_MAX];
    int LI[K_MAX];
#pragma unroll
    for (int s = 0; s < K_MAX; ++s) { L[s] = INFINITY; LI[s] = -1; }
    for (int sp = 0; sp < splits; ++sp) {
        const int64_t o = ((int64_t)sp * n_rows + i) * K_MAX;
#pragma unroll
        for (int s = 0; s < K_MAX; ++s) pair_insert(L, LI, lists[o + s], cols[o + s]);
    }
#pragma unroll
    for (int s = 0; s < K_MAX; ++s)
        if (s < k) { d2_out[i * k + s] = L[s]; idx_out[i * k + s] = LI[s]; }
}

// grid (column tiles, row blocks): z_out [n_rows][ceil(n_cols / 128) * 128], columns past n_cols not written
__global__ __launch_bounds__(THREADS, 2) void k_is_logits(Operands op, const float* __restrict__ bias, double* __restrict__ z_out)
{
    sweep<LOGIT>(op, 1, z_out, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, bias);
}

constexpr int IS_ROWS = 32;             // rows per block of k_is_rows: eight per wave, one after the other
constexpr int IS_MAX_CLASSES = 4096;
constexpr double IS_ONE = 4398046511104.0;      // 2^42 (NATINF_IS_FRAC_BITS)

// sum over the 64 lanes in a fixed tree; every lane returns the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s);
    return v;
}

// Block b: rows [32 b, 32 b + 32) of the staged logits z [n_rows][ldz]; wave w takes rows 32 b + w, + 4, ...  One wave per row, lane l the classes
// j = l, l + 64, ... in ascending order, three passes over the row (8 KB at 1,008 classes: the second and third are cache hits): the largest logit; the sum
// of exp(z - m) and the lowest class at m; p = exp(z - lse), the sum of p (z - lse) and q = llrint(2^42 p).  Every sum is the lanes' strided partial sums
// added in wave_sum's tree: a function of the row alone.  The q of the block's rows are added per class in LDS as integers (any order gives the same
// total), then one integer atomicAdd per class with a non-zero total goes into class_sums.
__global__ __launch_bounds__(THREADS) void k_is_rows(const double* __restrict__ z, int64_t ldz, int n_rows, int n_classes, double* __restrict__ neg_entropy,
                                                     double* __restrict__ lse_out, int* __restrict__ top_out, unsigned long long* __restrict__ class_sums)
{
    __shared__ unsigned long long sQ[IS_MAX_CLASSES];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int j = t; j < n_classes; j += THREADS) sQ[j] = 0ull;
    __syncthreads();
    for (int rr = w; rr < IS_ROWS; rr += THREADS / 64) {
        const int64_t i = (int64_t)blockIdx.x * IS_ROWS + rr;
        if (i >= n_rows) break;                                 // the wave's later rows lie further on
        const double* zr = z + i * ldz;
        double m = -INFINITY;
        for (int j = lane; j < n_classes; j += 64) m = fmax(m, zr[j]);
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) m = fmax(m, __shfl_xor(m, s));
        double se = 0.0;
        int top = n_classes;
        for (int j = lane; j < n_classes; j += 64) {
            const double v = zr[j];
            se += exp(v - m);
            top = (v == m && j < top) ? j : top;
        }
        se = wave_sum(se);
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) top = min(top, __shfl_xor(top, s));
        const double lse = m + log(se);
        double h = 0.0;
        for (int j = lane; j < n_classes; j += 64) {
            const double lp = zr[j] - lse;
            const double p = exp(lp);
            h += p * lp;
            const long long q = __double2ll_rn(p * IS_ONE);
            if (q) atomicAdd(&sQ[j], (unsigned long long)q);
        }
        h = wave_sum(h);
        if (lane == 0) {
            neg_entropy[i] = h;
            if (lse_out) lse_out[i] = lse;
            if (top_out) top_out[i] = top;
        }
    }
    __syncthreads();
    for (int j = t; j < n_classes; j += THREADS) {
        const unsigned long long v = sQ[j];
        if (v) atomicAdd(class_sums + j, v);
    }
}

}  // namespace prdc
