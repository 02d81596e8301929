/*
 * natinf_posterior.h -- C ABI of the posterior-concentration statistics inside libnatinf.so.
 *
 * Replaces the GPU statements of get_vp_statistics_tx / get_flow_statistics_tx (src/AnalyzeWeightedSumDegradation.py:93-108,
 * 135-146, 193-204): for one class of n feature vectors f_j (bf16 values, d each) and one noise level,
 *
 *   s_i  = fp32(fp32(f_i * a) + fp32(eps_i * b))                       the noised sample of row i (:98, :107)
 *   p_ij = softmax_j( -|s_i - f_j|^2 / (2 sigma^2) )                   in fp64 (:139-145)
 *   p_diag[i] = p_ii,  p_max[i] = max_j p_ij                           (:146-154)
 *
 * |s_i|^2 is constant along a row and drops out of the softmax, so p_ij = softmax_j((2 s_i.f_j - |f_j|^2) / (2 sigma^2)): one
 * GEMM and the row norms of f, no square root.  The fp32 s_i is split exactly into three bf16 terms hi + mid + lo (every residual
 * is exact in fp32), so s_i.f_j is three bf16 MFMA passes whose products are all exact in the fp32 accumulator; the accumulator is
 * added into an fp64 one after every 512 values of k, and everything after the GEMM is fp64.
 *
 * Shapes: 1 <= n <= 4096, d a multiple of 64, 64 <= d <= 65536.  The caller owns one workspace of
 * natinf_posterior_workspace_bytes(n, d) bytes (256-byte aligned device memory): the three planes, the row norms of f and the
 * GEMM's split-K partial sums.  natinf_posterior_samples fills the planes; natinf_posterior_stats, given the SAME n, d, features
 * and workspace afterwards on the same stream, writes the two statistics.  One samples call may be followed by any number of
 * stats calls (other sigmas).
 *
 * Every argument error is NATINF_EINVAL before anything is configured or launched (so also on a machine with no GPU);
 * NATINF_ELAUNCH when the runtime rejects a launch.
 */
#ifndef NATINF_POSTERIOR_H
#define NATINF_POSTERIOR_H

#include <stdint.h>
#include "natinf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NATINF_POSTERIOR_MAX_N 4096
#define NATINF_POSTERIOR_MAX_D 65536

/* bytes of the workspace for (n, d); negative (NATINF_EINVAL) for a shape outside the limits above.  Monotone in n and in d. */
int64_t natinf_posterior_workspace_bytes(int n, int d);

/* feats_bf16 [n][d] bf16 (device).  eps_i is row i of noise_or_null ([n][d] fp32, device) or, when that is NULL, what
 * natinf_randn_philox_f32(seed, global index of row i, elems_per_image = d) returns, bit for bit; the global index of row i is
 * index[i] (device int64 array) or, when index is NULL, first_index + i*index_stride.  The two products and the sum are three fp32
 * roundings, never contracted: the bytes of torch's `feats.float() * a + eps * b`.  The split into three bf16 terms is exact for
 * every finite s whose magnitude is at least 2^-100 (below that the last term can fall under bf16's subnormal step). */
int natinf_posterior_samples(const void* feats_bf16, const float* noise_or_null, float a, float b,
                             uint64_t seed, const int64_t* index, int64_t first_index, int64_t index_stride,
                             int n, int d, void* workspace, natinf_stream_t stream);

/* p_diag, p_max: [n] doubles (device).  sigma > 0 and finite.  Every value written is finite, in [0, 1], and p_max >= p_diag. */
int natinf_posterior_stats(const void* feats_bf16, double sigma, int n, int d, void* workspace,
                           double* p_diag, double* p_max, natinf_stream_t stream);

/* Test hook: s_out [n][d] fp32 (device) = hi + mid + lo of the planes the last natinf_posterior_samples(n, d) left in
 * `workspace`.  Runs on the null stream and waits for the device before and after. */
int natinf_posterior_debug_planes(const void* workspace, int n, int d, float* s_out);

#ifdef __cplusplus
}
#endif
#endif /* NATINF_POSTERIOR_H */
