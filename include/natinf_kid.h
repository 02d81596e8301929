/*
 * natinf_kid.h -- C ABI of the Kernel Inception Distance's device part inside libnatinf.so: per-row sums of the cubic polynomial
 * kernel (Binkowski et al. 2018; TF-GAN's kernel_classifier_distance) over a rows x columns matrix that is never stored.
 *
 *   s_ij    = a_i.b_j                          the distance kernels' own dot product (natinf_prdc.h): six bf16 MFMA passes over the
 *                                              planes of natinf_prdc_planes, exact products in an fp32 accumulator that is added into
 *                                              an fp64 one after every 64 values of k -- the same bytes as inside d2_ij
 *   k_ij    = u * u * u,  u = gamma * s_ij + coef0                                  in fp64
 *   sums[i] = sum of k_ij over the columns j < n_cols, j != self_offset + i         in fp64
 *
 * The unbiased MMD^2 of two sets is three such sums (set x set with self_offset, set x other), reduced and normalised on the host
 * (naturaldiffusion_amd/kid.py).  No norms are read.
 *
 * Determinism: sums[i] is a function of row i and of the column set only -- the same bytes for any split of the rows into calls or
 * ranks, and on every run.  The columns are cut into min(8, ceil(n_cols / 128)) ranges of whole 128-column tiles, a function of n_cols
 * alone; inside a range a row's columns fall into 64 classes (column mod 32, half of the tile), every class is added in ascending column
 * order, the classes in a fixed tree, the ranges in ascending order by a second kernel.  No floating-point atomics.
 *
 * Planes are taken in place: plane p of an operand starts p * plane_stride ELEMENTS after the pointer, so rows [s, s + n) of a set of N
 * rows prepared by natinf_prdc_planes are (planes + s * d, stride N * d, n).  `self_offset` as in natinf_prdc.h: >= 0 leaves column
 * self_offset + i out of row i (it needs self_offset + n_rows <= n_cols and n_cols >= 2), -1 leaves nothing out.
 *
 * Shapes: d a multiple of 64, 64 <= d <= 4096; 1 <= n_rows, n_cols <= 2^20; every stride a multiple of 8 and >= n * d; gamma and coef0
 * finite.  Planes are 16-byte aligned, sums_out 8-byte, the workspace 256-byte aligned device memory of at least
 * natinf_kid_workspace_bytes(n_rows, n_cols, d) bytes (one double per row and column range).
 *
 * Every argument error is NATINF_EINVAL before anything is configured or launched (so also on a machine with no GPU);
 * NATINF_ELAUNCH when the runtime rejects a launch.
 */
#ifndef NATINF_KID_H
#define NATINF_KID_H

#include <stdint.h>
#include "natinf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the workspace; negative (NATINF_EINVAL) for a shape outside the limits above.  Monotone in every argument. */
int64_t natinf_kid_workspace_bytes(int64_t n_rows, int64_t n_cols, int d);

/* sums_out [n_rows] fp64 (device), overwritten. */
int natinf_kid_row_sums(const void* row_planes, int64_t row_plane_stride, int64_t n_rows,
                        const void* col_planes, int64_t col_plane_stride, int64_t n_cols,
                        int d, int64_t self_offset, double gamma, double coef0,
                        double* sums_out, void* workspace, int64_t workspace_bytes, natinf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NATINF_KID_H */
