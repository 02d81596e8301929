/*
 * natinf_ideal.h -- C ABI of the ideal (empirical-Bayes) denoiser inside libnatinf.so: the posterior mean over a training set, the exact
 * minimum-MSE denoiser of the empirical training distribution, on the exact distance sweep of natinf_prdc.h.  It is the weighted sum
 * sum_j p_ij f_j whose concentration natinf_posterior.h measures, and a sampler that is KNOWN to copy its training set: the positive
 * control of natinf_nn.h's memorisation audit.  The rows x columns weight matrix is staged per chunk of rows, never stored whole.
 *
 * A training set is F [N][d] fp32, prepared once: natinf_prdc_planes (planes [3][N][d] and norms, natinf_prdc.h) and natinf_ideal_tplanes
 * (the same planes transposed, [3][d][Np] with Np = ceil(N / 64) * 64, pad columns zero).  A call takes query rows U [B][d] fp32 and a scale
 * c_i per row (fp64), and optionally x [B][d] fp32 with alpha_i, sigma_i (fp64, sigma_i > 0).
 *
 * Definition.
 *
 *   d2_ij   = the value every kernel of natinf_prdc.h forms for (u_i, f_j): byte for byte natinf_prdc_debug_dist2's; the left-out column
 *             self_offset + i, when self_offset >= 0, is +inf
 *   z_ij    = d2_ij == +inf ? -inf : -(c_i * d2_ij)                          fp64, one rounding
 *   m_i     = max_j z_ij ;  lse_i = m_i + log(sum_j exp(z_ij - m_i))         fp64, a fixed order: lane l of 64 adds the columns l, l + 64, ...
 *                                                                            in ascending order, the 64 partial sums in a fixed tree
 *   p_ij    = exp(z_ij - lse_i) ;  w_ij = fp32(p_ij)                         w split exactly into three bf16 planes hi + mid + lo
 *   mean_ie = sum_j w_ij f_je                                                the plane products hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi on the
 *                                                                            matrix cores, every product exact in an fp32 accumulator that is added
 *                                                                            into an fp64 one after every 64 values of j (the sweep's rule)
 *   x0_ie   = fp32(mean_ie)
 *   pmax_i  = exp(m_i - lse_i) ;  nearest_i = the lowest j with the smallest d2_ij        (chosen on d2, not on z; -1 when every d2 is +inf)
 *   out_ie  = fp32((x_ie - alpha_i * mean_ie) / sigma_i)                     fp64, every operation rounded once; only with x / alpha / sigma
 *
 * With u_i = x_i / alpha_i and c_i = alpha_i^2 / (2 sigma_i^2), x0 is E[x0 | x_t = x_i] for x_t = alpha f + sigma eps and a uniform prior on
 * the training set; out is that prediction in the eps form a score network returns, so natinf_step_f64hist recovers x0 from it with
 * std = sigma.
 *
 * Row function.  Every output of row i depends on row i, its scalars and the training set only: not on the other rows of the call, on how
 * the rows are split over calls or ranks, or on the launch geometry.  The reduction over j is split across blocks at fixed ranges of
 * NATINF_IDEAL_K_RANGE columns -- a function of N alone -- and the ranges' fp64 partial sums are added in ascending range order by a merge
 * kernel; no floating-point atomics.  The rows go through the staging buffers in chunks of NATINF_IDEAL_CHUNK_ROWS, which no output sees.
 *
 * The scales.  c, alpha and sigma are device arrays read by the kernels only, in stream order; their VALUES are not inspected (a read-back
 * would stall every step of a sampling job).  The contract is c_i >= 0 and finite.  What other values give: a NaN c_i makes x0, lse, pmax
 * and out of row i NaN (nearest_i, chosen on d2, is unaffected); a negative c_i gives the softmax of +|c_i| d2, which concentrates on the
 * FARTHEST rows; c_i = +inf gives NaN where some d2_ij is 0 and otherwise -inf logits throughout, hence NaN.  Other rows keep their bytes.
 * naturaldiffusion_amd.ideal.posterior_mean refuses such values wherever c is host data.
 *
 * Shapes: d a multiple of 64, 64 <= d <= 4096; 1 <= n_rows <= 2^20; 1 + (self_offset >= 0) <= n_cols <= 2^20; self_offset as in
 * natinf_prdc.h.  rows, planes and transposed planes are 16-byte aligned; c, alpha, sigma, norms, lse, pmax 8-byte; x, x0, out, nearest
 * 4-byte; the workspace 256-byte aligned device memory of at least natinf_ideal_workspace_bytes(n_rows, n_cols, d) bytes.
 *
 * Every argument error -- a NULL or misaligned pointer, a shape outside the limits, x given without alpha / sigma / out or the other way
 * round, a short workspace -- is NATINF_EINVAL before anything is configured or launched (so also on a machine with no GPU);
 * NATINF_ELAUNCH when the runtime rejects a launch.
 */
#ifndef NATINF_IDEAL_H
#define NATINF_IDEAL_H

#include <stdint.h>
#include "natinf.h"
#include "natinf_prdc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Columns j per block of the weighted sum: the split points of the reduction, a multiple of 64. */
#ifndef NATINF_IDEAL_K_RANGE
#define NATINF_IDEAL_K_RANGE 2048
#endif
/* Rows per pass through the staging buffers (distances, weight planes, partial sums), a multiple of 64. */
#ifndef NATINF_IDEAL_CHUNK_ROWS
#define NATINF_IDEAL_CHUNK_ROWS 256
#endif

/* planes [3][n][d] bf16 (natinf_prdc_planes) -> tplanes [3][d][np] bf16, np = ceil(n / 64) * 64, columns n .. np - 1 zero. */
int natinf_ideal_tplanes(const void* planes_bf16, int64_t n, int d, void* tplanes_bf16, natinf_stream_t stream);

/* bytes of the workspace; negative (NATINF_EINVAL) for a shape outside the limits above.  Monotone in every argument. */
int64_t natinf_ideal_workspace_bytes(int64_t n_rows, int64_t n_cols, int d);

/* rows [n_rows][d] fp32, c [n_rows] fp64; the training set's planes, norms and transposed planes.  x0_out [n_rows][d] fp32.  lse_out,
 * pmax_out (fp64 [n_rows]) and nearest_out (int32 [n_rows]) may each be NULL.  x [n_rows][d] fp32, alpha, sigma (fp64 [n_rows]) and
 * out [n_rows][d] fp32: all four given or all four NULL. */
int natinf_ideal_posterior_mean(const float* rows, const double* c, int64_t n_rows,
                                const void* col_planes, const double* col_norms, const void* col_tplanes, int64_t n_cols,
                                int d, int64_t self_offset,
                                const float* x, const double* alpha, const double* sigma,
                                float* x0_out, double* lse_out, double* pmax_out, int32_t* nearest_out, float* out,
                                void* workspace, int64_t workspace_bytes, natinf_stream_t stream);

/* Test hook: w_out [n_rows][n_cols] fp32 (device) = hi + mid + lo of the staged weight planes, n_rows * n_cols <= 2^20; planes_out, when
 * not NULL, receives the planes themselves, [3][n_rows][np] bf16 with their pad columns.  The workspace is natinf_ideal_posterior_mean's. */
int natinf_ideal_debug_weights(const float* rows, const double* c, int64_t n_rows,
                               const void* col_planes, const double* col_norms, int64_t n_cols,
                               int d, int64_t self_offset, float* w_out, void* planes_out,
                               void* workspace, int64_t workspace_bytes, natinf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NATINF_IDEAL_H */
