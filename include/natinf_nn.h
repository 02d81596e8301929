/*
 * natinf_nn.h -- C ABI of the nearest-neighbour search inside libnatinf.so: for every row the k nearest columns of a feature set, distances AND
 * indices, on the exact distance sweep of natinf_prdc.h (the memorisation audit: which training image is each generated image closest to?).
 * The rows x columns distance matrix is never stored.
 *
 * Feature sets are prepared by natinf_prdc_planes (natinf_prdc.h), whose limits, alignments and `self_offset` hold here unchanged.
 *
 * Definition.  Row i of the outputs holds the k smallest pairs (d2_ij, j) over the columns j in lexicographic order: ascending distance, and among
 * equal distances the lower column index first.  d2_ij = max(0, (|a_i|^2 + |b_j|^2) - 2 a_i.b_j) is the value every kernel of natinf_prdc.h forms
 * for (i, j): the same tile arithmetic, the same k order.  The left-out column (self_offset + i, when self_offset >= 0) and columns >= n_cols never
 * appear.
 *
 * Consistency.  d2_out[i][k - 1] equals natinf_prdc_knn_radius's r2_out[i] byte for byte, and every d2_out[i][t] equals natinf_prdc_debug_dist2's
 * entry at (i, idx_out[i][t]) byte for byte.
 *
 * Split invariance.  A row's result is a function of that row and of the column set only: not of how the rows are split over calls or ranks, of
 * the number of column ranges the call sweeps side by side, or of the launch geometry.  Ties included: every merge (the four column classes of a
 * row, the column ranges) compares (distance, index) pairs, never distances alone.
 *
 * Non-finite features.  An empty slot is the pair (+inf, -1), and only a pair below it enters a list: a column whose distance is +inf never does
 * (a NaN never reaches the comparison: the max(0, .) above turns it into 0, as in every kernel of natinf_prdc.h).  So an output slot that was
 * never filled holds d2 = +inf and idx = -1, and no index outside -1 .. n_cols - 1 is ever written.
 *
 * Shapes: d a multiple of 64, 64 <= d <= 4096; 1 <= k <= NATINF_PRDC_MAX_K; 1 <= n_rows <= 2^20; k + (self_offset >= 0) <= n_cols <= 2^20, so an
 * int32 index suffices.  Planes are 16-byte aligned, norms and d2_out 8-byte, idx_out 4-byte, the workspace 256-byte aligned device memory of at
 * least natinf_nn_workspace_bytes(n_rows, n_cols, d, k) bytes (linear in n_rows: the per-row pair lists of the column ranges).
 *
 * Every argument error -- a NULL or misaligned pointer, a shape outside the limits, a short workspace -- is NATINF_EINVAL before anything is
 * configured or launched (so also on a machine with no GPU); NATINF_ELAUNCH when the runtime rejects a launch.
 */
#ifndef NATINF_NN_H
#define NATINF_NN_H

#include <stdint.h>
#include "natinf.h"
#include "natinf_prdc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the workspace; negative (NATINF_EINVAL) for a shape outside the limits above.  Monotone in every argument. */
int64_t natinf_nn_workspace_bytes(int64_t n_rows, int64_t n_cols, int d, int k);

/* d2_out [n_rows][k] fp64 and idx_out [n_rows][k] int32 (device): the k nearest columns of every row, nearest first. */
int natinf_nn_nearest(const void* row_planes, const double* row_norms, int64_t n_rows,
                      const void* col_planes, const double* col_norms, int64_t n_cols,
                      int d, int k, int64_t self_offset,
                      double* d2_out, int32_t* idx_out,
                      void* workspace, int64_t workspace_bytes, natinf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NATINF_NN_H */
