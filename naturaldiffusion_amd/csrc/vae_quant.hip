// vae_quant.hip -- the AutoencoderKL encoder's quant_conv pass (vae_engine.inc, VaeEncBuilder): a translation unit of its own, next to ncsnpp.hip, whose
// kernel count tests/test_build_isa.py caps.  Tested alone against fp64 through natinf_debug_vae_quant (vae_engine.inc): tests/test_gpu_glue_kernels.py, N = 2 .. 64, hw = 1 / 63 / 64.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ncsn {

// quant_conv (1x1: W [N][N], bias) on the encoder's fp32 moments: m [B][N][hw] -> out [B][N][hw] (k_vae_latents' loop, fp32 in and out, no padding)
__global__ void k_vae_quant(const float* __restrict__ m, const float* __restrict__ W, const float* __restrict__ bias,
                            float* __restrict__ out, int N, int hw, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int p = (int)(i % hw), c = (int)((i / hw) % N); const int64_t b = i / ((int64_t)hw * N);
    float v = bias[c];
    for (int k = 0; k < N; ++k) v += W[c * N + k] * m[((int64_t)b * N + k) * hw + p];
    out[i] = v;
}

}  // namespace ncsn

namespace ncsn_vq {
__attribute__((visibility("hidden"))) void launch(const float* m, const float* W, const float* bias, float* out, int N, int hw, int64_t total, void* stream) {
    hipLaunchKernelGGL(ncsn::k_vae_quant, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, W, bias, out, N, hw, total);
}
}  // namespace ncsn_vq
