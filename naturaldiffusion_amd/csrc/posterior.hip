// posterior.hip -- the posterior statistics' GEMM, row reduction and test hook (posterior.h) and their C ABI (include/natinf_posterior.h).
// natinf_posterior_samples is in ni_step.hip, beside the Philox generator it must agree with bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "natinf.h"
#include "natinf_posterior.h"

namespace {
#include "posterior.h"
inline int launched() { return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH; }
}  // namespace

extern "C" {

int64_t natinf_posterior_workspace_bytes(int n, int d)
{
    if (!post::shape_ok(n, d)) return NATINF_EINVAL;
    return post::layout(n, d).total;
}

int natinf_posterior_stats(const void* feats_bf16, double sigma, int n, int d, void* workspace,
                           double* p_diag, double* p_max, natinf_stream_t stream)
{
    if (!feats_bf16 || !workspace || !p_diag || !p_max || !post::shape_ok(n, d) || !(sigma > 0.0) || !isfinite(sigma)) return NATINF_EINVAL;
    if (((uintptr_t)feats_bf16 & 15) || ((uintptr_t)workspace & 255)) return NATINF_EINVAL;
    const post::Layout L = post::layout(n, d);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    const __bf16* planes = reinterpret_cast<const __bf16*>(ws + L.planes);
    double* norms = reinterpret_cast<double*>(ws + L.norms);
    double* partial = reinterpret_cast<double*>(ws + L.partials);
    hipStream_t s = (hipStream_t)stream;

    hipLaunchKernelGGL(post::k_post_norms, dim3(n), dim3(post::THREADS), 0, s, (const post::bf16x8*)feats_bf16, norms, d / 8);
    if (launched() != NATINF_OK) return NATINF_ELAUNCH;
    const dim3 grid((n + post::BN - 1) / post::BN, (n + post::BM - 1) / post::BM, L.splits);
    hipLaunchKernelGGL(post::k_post_dots, grid, dim3(post::THREADS), 0, s, planes, (const __bf16*)feats_bf16, partial, n, d, L.splits);
    if (launched() != NATINF_OK) return NATINF_ELAUNCH;
    hipLaunchKernelGGL(post::k_post_rows, dim3(n), dim3(post::THREADS), 0, s, (const double*)partial, (const double*)norms, n, L.splits,
                       1.0 / (2.0 * sigma * sigma), p_diag, p_max);
    return launched();
}

int natinf_posterior_debug_planes(const void* workspace, int n, int d, float* s_out)
{
    if (!workspace || !s_out || !post::shape_ok(n, d) || ((uintptr_t)workspace & 255) || ((uintptr_t)s_out & 15)) return NATINF_EINVAL;
    const post::Layout L = post::layout(n, d);
    const int64_t nvec = (int64_t)n * d / 8;
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return NATINF_ELAUNCH; }
    hipLaunchKernelGGL(post::k_post_planes, dim3((unsigned)((nvec + post::THREADS - 1) / post::THREADS)), dim3(post::THREADS), 0, nullptr,
                       reinterpret_cast<const post::bf16x8*>(static_cast<const unsigned char*>(workspace) + L.planes), (float4*)s_out, nvec);
    if (launched() != NATINF_OK) return NATINF_ELAUNCH;
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return NATINF_ELAUNCH; }
    return NATINF_OK;
}

}  // extern "C"
