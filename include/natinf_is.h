/*
 * natinf_is.h -- C ABI of the Inception Score's device part inside libnatinf.so (Salimans et al. 2016; TF-GAN's
 * classifier_score_from_logits): per-row statistics of the softmax of feature rows against a classifier head, and the fixed-point
 * sum of the rows' class probabilities.
 *
 *   s_ij   = a_i.w_j          the distance kernels' own dot product (natinf_prdc.h): six bf16 MFMA passes over the planes of
 *                             natinf_prdc_planes, exact products in an fp32 accumulator that is added into an fp64 one after every
 *                             64 values of k -- the same bytes as inside d2_ij and k_ij
 *   z_ij   = s_ij + b_j                                                          fp64 (b_j = 0 without a bias)
 *   lse_i  = m_i + log(sum_j exp(z_ij - m_i)),  m_i = max_j z_ij                 fp64
 *   p_ij   = exp(z_ij - lse_i)
 *   h_i    = sum_j p_ij (z_ij - lse_i)          = sum_j p log p, the row's negative entropy      fp64
 *   top_i  = the lowest j with z_ij = m_i
 *   q_ij   = llrint(p_ij * 2^NATINF_IS_FRAC_BITS)                 int64;  Q_j = sum over the rows of q_ij
 *
 * The score of a set S of n rows is formed on the host (naturaldiffusion_amd/iscore.py):
 *
 *   pbar_j = Q_j / (n 2^42),   log IS = sum_i h_i / n - sum_{Q_j > 0} pbar_j log pbar_j,   IS = exp(log IS).
 *
 * Determinism: h_i, lse_i and top_i are functions of row i and of the head only -- the same bytes for any split of the rows into
 * calls or ranks, and on every run.  A row's sums over j are 64 strided partial sums (j = l, l + 64, ... in ascending order) added
 * in a fixed tree; no floating-point atomics.  The marginal is a sum over ROWS, so it is kept as integers: Q_j is the same
 * integer for any split, any order and any number of ranks (integer atomics, an integer all-reduce), at the price of at most 2^-43
 * of absolute error on every pbar_j.  With at most 2^20 rows added into one vector Q_j is 2^62 at the most.
 *
 * Planes are taken in place as in natinf_kid.h: plane p of an operand starts p * plane_stride ELEMENTS after the pointer.  The
 * logits of NATINF_IS_CHUNK_ROWS rows at a time are staged in the workspace as [rows][ceil(n_classes / 128) * 128] doubles,
 * written and read back once; no norms are read.
 *
 * Shapes: d a multiple of 64, 64 <= d <= 4096; 1 <= n_rows <= 2^20; 1 <= n_classes <= 4096; every stride a multiple of 8 and
 * >= n * d.  Planes are 16-byte aligned, the fp64 / int64 vectors 8-byte, bias and top_out 4-byte, the workspace 256-byte aligned
 * device memory of at least natinf_is_workspace_bytes(n_rows, n_classes, d) bytes.
 *
 * Every argument error is NATINF_EINVAL before anything is configured or launched (so also on a machine with no GPU);
 * NATINF_ELAUNCH when the runtime rejects a launch.
 */
#ifndef NATINF_IS_H
#define NATINF_IS_H

#include <stdint.h>
#include "natinf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NATINF_IS_FRAC_BITS  42
#define NATINF_IS_CHUNK_ROWS 8192
#define NATINF_IS_MAX_CLASSES 4096

/* bytes of the workspace: min(n_rows, NATINF_IS_CHUNK_ROWS) * ceil(n_classes / 128) * 128 * 8; negative (NATINF_EINVAL) for a
 * shape outside the limits above.  Monotone in every argument. */
int64_t natinf_is_workspace_bytes(int64_t n_rows, int n_classes, int d);

int natinf_is_row_stats(const void* row_planes, int64_t row_plane_stride, int64_t n_rows,
                        const void* head_planes, int64_t head_plane_stride, int n_classes, int d,
                        const float* bias,            /* [n_classes] device, or NULL */
                        double* neg_entropy_out,      /* [n_rows], overwritten */
                        double* lse_out,              /* [n_rows] or NULL */
                        int32_t* top_out,             /* [n_rows] or NULL */
                        int64_t* class_sums,          /* [n_classes], ADDED INTO: the caller zeroes it, and adds at most 2^20 rows into one vector */
                        void* workspace, int64_t workspace_bytes, natinf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NATINF_IS_H */
