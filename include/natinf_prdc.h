/*
 * natinf_prdc.h -- C ABI of the k-nearest-neighbour manifold metrics inside libnatinf.so: improved precision and recall
 * (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) on feature vectors such as Inception pool3.
 *
 * All four numbers are made of two per-row quantities over a rows x columns distance matrix that is never stored:
 *
 *   d2_ij          = max(0, (|a_i|^2 + |b_j|^2) - 2 a_i.b_j)                    in fp64
 *   r2[i]          = the k-th smallest d2_ij over the columns j                 (natinf_prdc_knn_radius)
 *   cnt_col_ball[i] = #{ j : d2_ij <= r2_cols[j] }   row i lies in column j's ball   (natinf_prdc_ball_counts)
 *   cnt_row_ball[i] = #{ j : d2_ij <= r2_rows[i] }   column j lies in row i's ball
 *
 * A feature set is prepared once by natinf_prdc_planes: the fp32 values split exactly into three bf16 terms hi + mid + lo (every
 * residual is exact in fp32) and the row norms in fp64.  a_i.b_j is six bf16 MFMA passes over the plane products hi.hi, hi.mid,
 * mid.hi, mid.mid, hi.lo, lo.hi (the three left out are below 2^-26 of |a_k b_k|); every product is exact in the fp32 accumulator,
 * which is added into an fp64 one after every 64 values of k; everything after the GEMM is fp64.
 *
 * A row's result is a function of that row and of the column set only -- not of the other rows of the call: the same bytes for any
 * split of the rows into calls or ranks.  `self_offset` >= 0 leaves column self_offset + i out of row i (a set against itself:
 * 0; rows [s, s + n_rows) of a set against the whole set: s; it needs self_offset + n_rows <= n_cols); -1 leaves nothing out.
 *
 * Shapes: d a multiple of 64, 64 <= d <= 4096; 1 <= k <= 8; 1 <= n_rows <= 2^20; k + (self_offset >= 0) <= n_cols <= 2^20.
 * Planes are 16-byte aligned, norms / radii 8-byte, counts 4-byte, the workspace of natinf_prdc_knn_radius 256-byte aligned device
 * memory of at least natinf_prdc_workspace_bytes(n_rows, n_cols, d, k) bytes (linear in n_rows: the per-row lists of the column splits).
 *
 * Every argument error is NATINF_EINVAL before anything is configured or launched (so also on a machine with no GPU);
 * NATINF_ELAUNCH when the runtime rejects a launch.
 */
#ifndef NATINF_PRDC_H
#define NATINF_PRDC_H

#include <stdint.h>
#include "natinf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NATINF_PRDC_MAX_N (1 << 20)
#define NATINF_PRDC_MAX_D 4096
#define NATINF_PRDC_MAX_K 8

/* bytes of the workspace; negative (NATINF_EINVAL) for a shape outside the limits above.  Monotone in every argument. */
int64_t natinf_prdc_workspace_bytes(int64_t n_rows, int64_t n_cols, int d, int k);

/* feats [n][d] fp32 (device) -> planes_bf16 [3][n][d] and norms [n] (fp64: the fixed-tree sum of (double)x * (double)x).
 * hi + mid + lo == x exactly for every finite x whose magnitude is at least 2^-100. */
int natinf_prdc_planes(const float* feats, int64_t n, int d, void* planes_bf16, double* norms, natinf_stream_t stream);

/* r2_out [n_rows]: the k-th smallest d2_ij of row i. */
int natinf_prdc_knn_radius(const void* row_planes, const double* row_norms, int64_t n_rows,
                           const void* col_planes, const double* col_norms, int64_t n_cols,
                           int d, int k, int64_t self_offset, double* r2_out,
                           void* workspace, int64_t workspace_bytes, natinf_stream_t stream);

/* cnt_row_ball needs r2_rows [n_rows], cnt_col_ball needs r2_cols [n_cols]; either pair may be NULL (both members), not both pairs.
 * Comparisons are `<=` in fp64.  The left-out column is not counted.  int32 [n_rows] each, overwritten (the call zeroes them and the
 * column splits add into them: integer sums, the same in any order -- no workspace). */
int natinf_prdc_ball_counts(const void* row_planes, const double* row_norms, int64_t n_rows,
                            const void* col_planes, const double* col_norms, int64_t n_cols,
                            int d, int64_t self_offset, const double* r2_rows, const double* r2_cols,
                            int32_t* cnt_row_ball, int32_t* cnt_col_ball, natinf_stream_t stream);

/* Test hook: d2_out [n_rows][n_cols] fp64 (device) by the same tile arithmetic, the left-out column +inf; n_rows * n_cols <= 2^20. */
int natinf_prdc_debug_dist2(const void* row_planes, const double* row_norms, int64_t n_rows,
                            const void* col_planes, const double* col_norms, int64_t n_cols,
                            int d, int64_t self_offset, double* d2_out, natinf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NATINF_PRDC_H */
