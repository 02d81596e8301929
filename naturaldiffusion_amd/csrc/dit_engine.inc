// dit_engine.inc -- DiT denoiser engine (C ABI of include/natinf_dit.h); included at the end of ncsnpp.hip: one translation
// unit with the GEMM launch layer (gemm_launch.h), the engine base (engine_core.h) and the packing kernels.
//
// One forward = patch-embed(+pos) -> conditioning (t-MLP + label row -> SiLU) -> ONE GEMM for every block's adaLN
// modulation (6*depth+2 vectors per sample) -> depth x { LN+modulate, q|k GEMM, V^T GEMM, per-head QK^T / softmax /
// PV, proj GEMM with gate*(.)+x epilogue, LN+modulate, fc1 GEMM + GELU(tanh), fc2 GEMM with gate*(.)+x epilogue }
// -> LN+modulate -> linear -> unpatchify.  Residual stream fp32, GEMM operands bf16.
// NATINF_DIT_FP8: the q | k | v, fc1 and fc2 GEMMs of every block on e4m3 operands (include/natinf_dit.h states the arithmetic); everything else as above.
// Reference: deps/DiT/models.py:19-20,27-99,105-146,222-253,279-326.
#include "natinf_dit.h"
#include "engine_core.h"
#include "attn_fused.h"
#include "dit_flash.h"

namespace ncsn {

// x[b*T + t][d] = sum_k W[d][k] * patch(b, t)[k] + bias[d] + pos[t][d];  k = (c, pi, qi) as Conv2d(p, stride p) flattens
// z [B][C][2g][2g], patch 2, g x g tokens per sample; Wt = the conv weight TRANSPOSED to [C*4][D].  A block owns 256
// output channels of PE_TOK consecutive tokens: the 4C patch values of those tokens are staged in LDS once, every weight
// is read once per block (coalesced) and reused for all PE_TOK tokens from a register.
constexpr int PE_TOK = 16;
template <bool XH = false>                                                 // XH: x is written as IEEE half (the MMDiT engine's 16-bit image stream)
__global__ __launch_bounds__(256) void k_patch_embed(const float* __restrict__ z, const float* __restrict__ Wt,
                                                     const float* __restrict__ bias, const float* __restrict__ pos,
                                                     float* __restrict__ x, int C, int g, int D, int64_t rows)
{
    __shared__ float sp[PE_TOK][64];                                      // C*4 <= 64 patch values per token
    lds_poison();
    const int K = C * 4, T = g * g, S = 2 * g;
    const int64_t row0 = (int64_t)blockIdx.y * PE_TOK;
    const int d = blockIdx.x * 256 + threadIdx.x;
    for (int e = threadIdx.x; e < PE_TOK * K; e += 256) {
        const int tk = e / K, k = e - tk * K, c = k >> 2, pi = (k >> 1) & 1, qi = k & 1;
        const int64_t row = min(row0 + tk, rows - 1);
        const int t = (int)(row % T), gh = t / g, gw = t - gh * g; const int64_t b = row / T;
        sp[tk][k] = z[(((int64_t)b * C + c) * S + gh * 2 + pi) * S + gw * 2 + qi];
    }
    __syncthreads();
    if (d >= D) return;
    float acc[PE_TOK];
    const float bv = bias[d];
#pragma unroll
    for (int tk = 0; tk < PE_TOK; ++tk) acc[tk] = bv;
    for (int k = 0; k < K; ++k) {
        const float w = Wt[(int64_t)k * D + d];
#pragma unroll
        for (int tk = 0; tk < PE_TOK; ++tk) acc[tk] += w * sp[tk][k];
    }
#pragma unroll
    for (int tk = 0; tk < PE_TOK; ++tk) {
        const int64_t row = row0 + tk;
        if (row < rows) {
            const float v = acc[tk] + pos[(row % T) * D + d];
            if constexpr (XH) reinterpret_cast<_Float16*>(x)[row * D + d] = (_Float16)v; else x[row * D + d] = v;
        }
    }
}
// the patch embedding of a plan: plain or guarded (guard: the site's slot), onto an fp32 or a half stream
inline void launch_patch_embed(const float* z, const float* Wt, const float* bias, const float* pos, float* x, int C, int g, int D, int64_t rows, bool x_f16, uint32_t* guard, hipStream_t s)
{
    const dim3 grid((unsigned)((D + 255) / 256), (unsigned)((rows + PE_TOK - 1) / PE_TOK));
    if (guard) ncsn_sg::launch_patch_embed(z, Wt, bias, pos, x, C, g, D, rows, x_f16, guard, (void*)s);      // k_patch_embed_guard (stream_guard.hip)
    else if (x_f16) hipLaunchKernelGGL(k_patch_embed<true>, grid, dim3(256), 0, s, z, Wt, bias, pos, x, C, g, D, rows);
    else hipLaunchKernelGGL(k_patch_embed<false>, grid, dim3(256), 0, s, z, Wt, bias, pos, x, C, g, D, rows);
}
// timestep frequency embedding [B][256] = [cos | sin] (models.py:41-58)
__global__ void k_dit_time_freq(const float* __restrict__ t, bf16* __restrict__ emb, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * 256) return;
    const int b = i >> 8, j = i & 255, h = j & 127;
    const float a = t[b] * expf(-9.210340371976184f * (float)h / 128.0f);
    emb[i] = (bf16)(j < 128 ? cosf(a) : sinf(a));
}

// cs[b][d] = SiLU(c0[b][d] + table[y[b]][d]) as bf16: the input of every adaLN_modulation Linear
__global__ void k_dit_cond(const float* __restrict__ c0, const float* __restrict__ table, const int32_t* __restrict__ y,
                           bf16* __restrict__ cs, int D, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D) return;
    const int b = i / D, d = i - b * D;
    cs[i] = (bf16)silu_f(c0[i] + table[(int64_t)y[b] * D + d]);
}

// h = LayerNorm(x) * (1 + scale[b]) + shift[b]  (no affine, eps 1e-6); one wave per token row, fp32 statistics
// (x_f16: the residual stream is IEEE half -- the MMDiT engine's 16-bit image stream, natinf_set_mmdit_stream16 -- read through the same pointer)
__global__ __launch_bounds__(256) void k_ln_modulate(const float* __restrict__ x, const float* __restrict__ shift,
                                                     const float* __restrict__ scale, int mod_ld, bf16* __restrict__ h,
                                                     int D, int64_t rows, int rows_per_sample, int x_f16 = 0)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * D;
    const _Float16* xh = reinterpret_cast<const _Float16*>(x) + row * D;
    float v[24];                                                    // D <= 1536
    const int n = D >> 6;
    float s = 0.f;
    for (int i = 0; i < n; ++i) { v[i] = x_f16 ? (float)xh[lane + 64 * i] : xr[lane + 64 * i]; s += v[i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)D;
    float q = 0.f;
    for (int i = 0; i < n; ++i) { const float d = v[i] - mean; q += d * d; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / sqrtf(q / (float)D + 1e-6f);
    const int64_t b = row / rows_per_sample;
    const float* sh = shift + b * mod_ld; const float* sc = scale + b * mod_ld;
    for (int i = 0; i < n; ++i) {
        const int d = lane + 64 * i;
        h[row * D + d] = (bf16)((v[i] - mean) * rstd * (1.0f + sc[d]) + sh[d]);
    }
}
// The same for D = NC * 256 (SD3: 1536): a lane owns four consecutive columns per 256-column chunk -- 16-byte loads of x, scale and shift,
// 8-byte stores, everything unrolled.  The scalar form above moved 300 MB per SD3 image-stream launch at 2.4 TB/s (8 % of the forward,
// profiles/r02/sd3_kernel_stats.csv): one 4-byte load per lane and instruction, three loads per element.
// XH: x is IEEE half (8-byte loads of four columns; the statistics and the modulation stay fp32)
template <int NC, int REM = 0, bool XH = false>          // D = NC * 256 + REM; REM % 4 == 0: the last, partial chunk is owned by lanes 0 .. REM / 4 - 1 (DiT-XL/2: 1152 = 4 * 256 + 128)
__global__ __launch_bounds__(256) void k_ln_modulate_v4(const float* __restrict__ x, const float* __restrict__ shift,
                                                        const float* __restrict__ scale, int mod_ld, bf16* __restrict__ h,
                                                        int64_t rows, int rows_per_sample)
{
    constexpr int D = NC * 256 + REM, NV = NC + (REM ? 1 : 0);
    static_assert(REM % 4 == 0 && REM < 256, "a partial chunk of whole float4s");
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const bool tail = lane < REM / 4;                                   // this lane owns columns of the partial chunk
    const float4* xr = reinterpret_cast<const float4*>(x + row * D) + lane;
    const uint2* xh = reinterpret_cast<const uint2*>(reinterpret_cast<const _Float16*>(x) + row * D) + lane;
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if constexpr (XH) {
            typedef _Float16 f16x4_ln __attribute__((ext_vector_type(4)));
            const f16x4_ln hv = (i < NC || tail) ? __builtin_bit_cast(f16x4_ln, xh[64 * i]) : f16x4_ln{0, 0, 0, 0};
            v[i] = make_float4((float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]);
        } else v[i] = (i < NC || tail) ? xr[64 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (i < NC || tail) {
            const float a = v[i].x - mean, b_ = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + b_ * b_) + (c * c + d * d);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / sqrtf(q / (float)D + 1e-6f);
    const int64_t b = row / rows_per_sample;
    const float4* sh = reinterpret_cast<const float4*>(shift + b * mod_ld) + lane;
    const float4* sc = reinterpret_cast<const float4*>(scale + b * mod_ld) + lane;
    uint2* out = reinterpret_cast<uint2*>(h + row * D) + lane;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (i < NC || tail) {
            const float4 g = sc[64 * i], t = sh[64 * i];
            bf16x4_t o;
            o[0] = (bf16)((v[i].x - mean) * rstd * (1.0f + g.x) + t.x); o[1] = (bf16)((v[i].y - mean) * rstd * (1.0f + g.y) + t.y);
            o[2] = (bf16)((v[i].z - mean) * rstd * (1.0f + g.z) + t.z); o[3] = (bf16)((v[i].w - mean) * rstd * (1.0f + g.w) + t.w);
            out[64 * i] = __builtin_bit_cast(uint2, o);
        }
    }
}
// The half stream in 16-byte accesses (D = NC8 * 512; SD3: 1536): a lane owns EIGHT consecutive columns per 512-column chunk -- one 16-byte load of x, two of scale and of
// shift, one 16-byte store of h.  Alone it takes 35 us per SD3 image-stream launch (200 MB: 5.7 TB/s); inside a forward its mean is ~50 us like the four-column form's
// (51.6 us: profiles/r06/sd3_kernel_stats.csv) -- the text stream's GEMMs run beside it on their own HIP stream (min 35, max 79 us over a forward's 96 launches).
// Same arithmetic per element; the row statistics are summed in another order (fp32: last-bit differences).
template <int NC8>
__global__ __launch_bounds__(256) void k_ln_modulate_h8(const float* __restrict__ x, const float* __restrict__ shift, const float* __restrict__ scale, int mod_ld,
                                                        bf16* __restrict__ h, int64_t rows, int rows_per_sample)
{
    constexpr int D = NC8 * 512;
    typedef _Float16 f16x8_ln __attribute__((ext_vector_type(8)));
    typedef __bf16 bf16x8_ln __attribute__((ext_vector_type(8)));
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint4* xh = reinterpret_cast<const uint4*>(reinterpret_cast<const _Float16*>(x) + row * D) + lane;
    float v[NC8][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NC8; ++i) {
        const f16x8_ln hv = __builtin_bit_cast(f16x8_ln, xh[64 * i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = (float)hv[e];
        s += ((v[i][0] + v[i][1]) + (v[i][2] + v[i][3])) + ((v[i][4] + v[i][5]) + (v[i][6] + v[i][7]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NC8; ++i) {
        float d[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = v[i][e] - mean;
        q += ((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) + ((d[4] * d[4] + d[5] * d[5]) + (d[6] * d[6] + d[7] * d[7]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / sqrtf(q / (float)D + 1e-6f);
    const int64_t b = row / rows_per_sample;
    const float4* sh = reinterpret_cast<const float4*>(shift + b * mod_ld) + 2 * lane;
    const float4* sc = reinterpret_cast<const float4*>(scale + b * mod_ld) + 2 * lane;
    uint4* out = reinterpret_cast<uint4*>(h + row * D) + lane;
#pragma unroll
    for (int i = 0; i < NC8; ++i) {
        const float4 g0 = sc[128 * i], g1 = sc[128 * i + 1], t0 = sh[128 * i], t1 = sh[128 * i + 1];
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, tt[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
        bf16x8_ln o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)((v[i][e] - mean) * rstd * (1.0f + gg[e]) + tt[e]);
        out[64 * i] = __builtin_bit_cast(uint4, o);
    }
}
// Returns the form it launched -- 0 scalar, 1 four-column, 2 eight-column -- for natinf_debug_ln_modulate (tests/test_gpu_row_kernels.py); the engines ignore it.
inline int launch_ln_modulate(const float* x, const float* shift, const float* scale, int mod_ld, bf16* h, int D, int64_t rows, int rows_per_sample,
                              hipStream_t s, bool x_f16 = false)
{
    const dim3 grid((unsigned)((rows + 3) / 4));
    const bool al = mod_ld % 4 == 0 && (reinterpret_cast<uintptr_t>(shift) | reinterpret_cast<uintptr_t>(scale)) % 16 == 0;
    if (x_f16) {                                                        // the MMDiT engine's 16-bit image stream
        if (D == 1536 && al) { hipLaunchKernelGGL(k_ln_modulate_h8<3>, grid, dim3(256), 0, s, x, shift, scale, mod_ld, h, rows, rows_per_sample); return 2; }
        if (D == 256 && al) { hipLaunchKernelGGL((k_ln_modulate_v4<1, 0, true>), grid, dim3(256), 0, s, x, shift, scale, mod_ld, h, rows, rows_per_sample); return 1; }
        if (D == 1152 && al) { hipLaunchKernelGGL((k_ln_modulate_v4<4, 128, true>), grid, dim3(256), 0, s, x, shift, scale, mod_ld, h, rows, rows_per_sample); return 1; }      // DiT-XL/2
        hipLaunchKernelGGL(k_ln_modulate, grid, dim3(256), 0, s, x, shift, scale, mod_ld, h, D, rows, rows_per_sample, 1);
        return 0;
    }
    if (D == 1536 && al) { hipLaunchKernelGGL(k_ln_modulate_v4<6>, grid, dim3(256), 0, s, x, shift, scale, mod_ld, h, rows, rows_per_sample); return 1; }
    if (D == 256 && al) { hipLaunchKernelGGL(k_ln_modulate_v4<1>, grid, dim3(256), 0, s, x, shift, scale, mod_ld, h, rows, rows_per_sample); return 1; }
    if (D == 1152 && al) { hipLaunchKernelGGL((k_ln_modulate_v4<4, 128>), grid, dim3(256), 0, s, x, shift, scale, mod_ld, h, rows, rows_per_sample); return 1; }      // DiT-XL/2
    hipLaunchKernelGGL(k_ln_modulate, grid, dim3(256), 0, s, x, shift, scale, mod_ld, h, D, rows, rows_per_sample, 0);
    return 0;
}

// out[n][c][gh*2+pi][gw*2+qi] = tok[n*g*g + gh*g+gw][(pi*2+qi)*OC + c]   (models.py:222-235)
__global__ void k_unpatchify(const float* __restrict__ tok, float* __restrict__ out, int OC, int g, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int S = 2 * g, xw = (int)(i % S), yh = (int)((i / S) % S), c = (int)((i / ((int64_t)S * S)) % OC); const int64_t n = i / ((int64_t)S * S * OC);
    out[i] = tok[(n * g * g + (yh >> 1) * g + (xw >> 1)) * (4 * OC) + ((yh & 1) * 2 + (xw & 1)) * OC + c];
}
// k_softmax_rows for the per-head attention path at more than 256 keys (DiT at input 64: 1,024): one wave per row, T % 64 == 0, T <= 1024
__global__ __launch_bounds__(256) void k_softmax_rows_1k(const float* __restrict__ S, bf16* __restrict__ P, int T, int64_t rows)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* s = S + row * T;
    const int n = T >> 6;
    float v[16];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) { v[i] = i < n ? s[lane + 64 * i] : -INFINITY; mx = fmaxf(mx, v[i]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { v[i] = i < n ? __expf(v[i] - mx) : 0.f; sum += v[i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i < n) P[row * T + lane + 64 * i] = (bf16)(v[i] * inv);
}
__global__ void k_f32_to_bf16(const float* __restrict__ src, bf16* __restrict__ dst, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (bf16)src[i];
}
// cs[i] = SiLU(c[i]) as bf16
__global__ void k_silu_bf16(const float* __restrict__ c, bf16* __restrict__ cs, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cs[i] = (bf16)silu_f(c[i]);
}

}  // namespace ncsn

struct natinf_dit : EngineCore {
    int depth = 0, D = 0, heads = 0, hd = 0, nmod = 0;
    int input_size = 32, T = 256;        // latent side S and tokens (S / 2)^2: natinf_dit_create_sized
    const int32_t* y = nullptr;          // per-forward
    bool unfused_attention = false;      // NATINF_DIT_UNFUSED_ATTENTION: per-head GEMM / softmax / GEMM (also used when head_dim > 96)
    bool fp8 = false;                    // NATINF_DIT_FP8: q | k | v, fc1 and fc2 on e4m3 operands (weights: a scale per output channel; LN-modulate rows: a scale per token; GELU(fc1): E8M0 block scales)
    bool stream16 = false;               // natinf_set_dit_stream16 (read when the plan is BUILT): the residual stream x [T][D] in IEEE half, not fp32 (as the MMDiT engine's image stream)
    // NATINF_DIT_STREAM_GUARD: EngineCore::guard_sites = 1 + 2 depth -- the patch embedding (site 0), then per block the attention-projection update (1 + 2 i) and the MLP update (2 + 2 i)
};

namespace {

constexpr int DIT_STREAM16_DEFAULT = 1;          // (round 6: DiT-XL/2 forward of 16 6.53 -> 6.28 ms; profiles/r06/dit_stream16_ab.txt)
int g_dit_stream16 = DIT_STREAM16_DEFAULT;      // natinf_set_dit_stream16

// qkv: [B*256][3 D] (q | k | v columns, one GEMM); v is transposed inside the attention kernel on its way into LDS (k_attn_fused<., ., false, true>).
// More than 256 tokens: the streaming kernel of dit_flash.h on the same buffer (launch_dit_flash).
template <int NQK, int ND>
void launch_attn(const bf16* qkv, bf16* o, int B, int D, int H, int hd, hipStream_t s) {
    using Cfg = AttnCfg<NQK, ND>;
    auto kern = &k_attn_fused<NQK, ND, false, true>;
    hipLaunchKernelGGL(kern, dim3((unsigned)(B * H)), dim3(Cfg::THREADS), Cfg::LDS_BYTES, s, qkv, 3 * D, D, qkv + 2 * D, o, D, H, hd,
                       1.0f / sqrtf((float)hd));
}
bool configure_dit_attention() {      // (k_attn_fused<2,4> / <3,5> / <3,6> with v as V^T: superseded by these row-major-v forms)
    return set_lds<AttnCfg<2, 4>>(&k_attn_fused<2, 4, false, true>) && set_lds<AttnCfg<3, 5>>(&k_attn_fused<3, 5, false, true>) &&
           set_lds<AttnCfg<3, 6>>(&k_attn_fused<3, 6, false, true>);
}

struct DitBuilder : PlanBuilder {
    natinf_dit& E;
    explicit DitBuilder(natinf_dit& e) : PlanBuilder(e), E(e) {}
    void build() {
        const int D = E.D, H = E.heads, hd = E.hd, T = E.T, depth = E.depth, gs = E.input_size / 2;       // gs: tokens per latent side
        const int log_T = T == 256 ? 8 : 10;                        // rows per sample of the gated epilogues (256 or 1,024 tokens)
        const int nmod = (6 * depth + 2) * D;
        E.nmod = nmod;
        // ---- parameters (order documented in natinf_dit.h)
        const int64_t p_pos = take((int64_t)T * D), p_pw = take((int64_t)D * 16), p_pb = take(D);
        const int64_t p_t0w = take((int64_t)D * 256), p_t0b = take(D), p_t2w = take((int64_t)D * D), p_t2b = take(D);
        const int64_t p_tab = take((int64_t)1001 * D);
        const int64_t w_pos = pack_f32(p_pos, (int64_t)T * D), w_pw = pack_f32_transposed(p_pw, D, 16), w_pb = pack_f32(p_pb, D);
        const int64_t w_t0 = pack_bf16(p_t0w, D, 256), b_t0 = pack_f32(p_t0b, D), w_t2 = pack_bf16(p_t2w, D, D), b_t2 = pack_f32(p_t2b, D);
        const int64_t w_tab = pack_f32(p_tab, (int64_t)1001 * D);
        const int64_t w_mod = wres((int64_t)nmod * D * 2), b_mod = wres((int64_t)nmod * 4);     // all adaLN linears, stacked

        // ---- workspace (bytes per image)
        const bool fused_attn = hd <= 96 && !E.unfused_attention;
        // fused attention: q | k | v of a block are ONE GEMM into [T][3 D]; the per-head GEMM path keeps q | k and the batched V^T = W_v h^T GEMM
        const int QL = fused_attn ? 3 * D : 2 * D;
        const bool s16 = E.stream16;                                // the residual stream in IEEE half (the update stays fp32, one rounding per update)
        const int64_t x = arena.alloc((int64_t)T * D * (s16 ? 2 : 4)), h = arena.alloc((int64_t)T * D * 2), qk = arena.alloc((int64_t)T * QL * 2);
        const int64_t vT = fused_attn ? 0 : arena.alloc((int64_t)D * T * 2);
        const int64_t S = fused_attn ? 0 : arena.alloc((int64_t)H * T * T * 4), P = fused_attn ? 0 : arena.alloc((int64_t)H * T * T * 2);
        const bool fp8 = E.fp8;
        const int64_t o = arena.alloc((int64_t)T * D * 2), f = fp8 ? 0 : arena.alloc((int64_t)T * 4 * D * 2), mod = arena.alloc((int64_t)nmod * 4);
        // fp8 mode: LN-modulate rows as e4m3 + a scale per token; GELU(fc1) as e4m3 + one E8M0 scale per 32 columns, K-tile-major planes of B * T rows (ncsnpp_kernels.h).
        // Every GEMM here has M = B * T rows, a whole number of 256-row tiles, and an attention launch is one (sample, head) of exactly T rows: no kernel reads an fp8 / MX
        // operand beyond the rows the same forward wrote, so nothing has to be zeroed (the MMDiT's padded joint sequence does: mmdit_engine.inc).
        const int64_t h8 = fp8 ? arena.alloc((int64_t)T * D) : 0, sx = fp8 ? arena.alloc((int64_t)T * 4) : 0;
        const int64_t f8 = fp8 ? arena.alloc((int64_t)T * 4 * D) : 0, fmx = fp8 ? arena.alloc((int64_t)T * 4 * D / 32) : 0;
        constexpr int SK_MAX = 4;                                   // split-K slices of fc2 at small batches (launch_gemm decides: w128_splitk_slices)
        const int64_t skw = arena.alloc((int64_t)SK_MAX * T * D * 4);
        const int64_t tf = arena.alloc(256 * 2), t1 = arena.alloc((int64_t)D * 2), c0 = arena.alloc((int64_t)D * 4), cs = arena.alloc((int64_t)D * 2);
        const int64_t tok = arena.alloc((int64_t)T * 32 * 4);

        natinf_dit* eng = &E;
        op([=](const Ctx& c) {                                      // embeddings and conditioning
            const int64_t prow = (int64_t)c.B * T;
            launch_patch_embed(c.x, c.w<float>(w_pw), c.w<float>(w_pb), c.w<float>(w_pos), c.at<float>(x), 4, gs, D, prow, s16, c.site(0), c.stream);
            hipLaunchKernelGGL(k_dit_time_freq, dim3(grid1d((int64_t)c.B * 256)), dim3(256), 0, c.stream, c.labels, c.at<bf16>(tf), c.B);
            GemmArgs g = gemm_defaults();                           // SiLU(Linear_0(t_freq))
            g.a0 = c.at<bf16>(tf); g.a0_ld = 256; g.a0_C = 256; g.M = c.B; g.N = D; g.b = c.w<bf16>(w_t0); g.b_ld = 256;
            g.bias_n = c.w<float>(b_t0); g.act = ACT_SILU; g.c = c.at<bf16>(t1); g.c_ld = D;
            launch_gemm(g, c.stream);
            g = gemm_defaults();                                    // Linear_2(.) -> fp32
            g.a0 = c.at<bf16>(t1); g.a0_ld = D; g.a0_C = D; g.M = c.B; g.N = D; g.b = c.w<bf16>(w_t2); g.b_ld = D;
            g.bias_n = c.w<float>(b_t2); g.c = c.at<float>(c0); g.c_ld = D; g.c_mode = OUT_F32;
            launch_gemm(g, c.stream);
            hipLaunchKernelGGL(k_dit_cond, dim3(grid1d((int64_t)c.B * D)), dim3(256), 0, c.stream, c.at<float>(c0), c.w<float>(w_tab),
                               eng->y, c.at<bf16>(cs), D, c.B);
            g = gemm_defaults();                                    // every adaLN_modulation Linear at once
            g.a0 = c.at<bf16>(cs); g.a0_ld = D; g.a0_C = D; g.M = c.B; g.N = nmod; g.b = c.w<bf16>(w_mod); g.b_ld = D;
            g.bias_n = c.w<float>(b_mod); g.c = c.at<float>(mod); g.c_ld = nmod; g.c_mode = OUT_F32;
            launch_gemm(g, c.stream);
        });

        auto ln_mod = [=](int shift_off, int scale_off) {
            return [=](const Ctx& c) {
                const int64_t rows = (int64_t)c.B * T;
                launch_ln_modulate(c.at<float>(x), c.at<float>(mod) + shift_off, c.at<float>(mod) + scale_off, nmod, c.at<bf16>(h), D, rows, T, c.stream, s16);
            };
        };

        auto ln_mod8 = [=](int shift_off, int scale_off) {         // -> e4m3 rows + per-token scales
            return [=](const Ctx& c) {
                launch_ln_modulate_fp8(c.at<float>(x), c.at<float>(mod) + shift_off, c.at<float>(mod) + scale_off, nmod, c.at<uint8_t>(h8), c.at<float>(sx), D, (int64_t)c.B * T, T,
                                       c.stream, s16);
            };
        };
        auto pack8 = [&](int64_t src, int rows, int cols) {          // e4m3 bytes [rows][cols] + one scale per row: {weights, scales}
            const std::pair<int64_t, int64_t> r{wres((int64_t)rows * cols), wres((int64_t)rows * 4)};
            pack_fp8_at(src, rows, cols, r.first, r.second);
            return r;
        };

        for (int i = 0; i < depth; ++i) {
            const int64_t p_qkvw = take((int64_t)3 * D * D), p_qkvb = take(3 * D), p_pw2 = take((int64_t)D * D), p_pb2 = take(D);
            const int64_t p_f1w = take((int64_t)4 * D * D), p_f1b = take(4 * D), p_f2w = take((int64_t)4 * D * D), p_f2b = take(D);
            const int64_t p_mw = take((int64_t)6 * D * D), p_mb = take(6 * D);
            // (the checkpoint's qkv rows are q, k, v in this order)      fp8: {e4m3 bytes, per-output-channel scales} in place of the bf16 matrix
            const std::pair<int64_t, int64_t> q8 = fp8 ? pack8(p_qkvw, QL, D) : std::pair<int64_t, int64_t>{0, 0};
            const std::pair<int64_t, int64_t> v8 = fp8 && !fused_attn ? pack8(p_qkvw + (int64_t)2 * D * D, D, D) : std::pair<int64_t, int64_t>{0, 0};
            const int64_t w_qk = fp8 ? q8.first : pack_bf16(p_qkvw, QL, D), s_qk = q8.second, b_qk = pack_f32(p_qkvb, QL);
            const int64_t w_v = fused_attn ? 0 : (fp8 ? v8.first : pack_bf16(p_qkvw + (int64_t)2 * D * D, D, D)), s_v = v8.second, b_v = fused_attn ? 0 : pack_f32(p_qkvb + 2 * D, D);
            const int64_t w_pr = pack_bf16(p_pw2, D, D), b_pr = pack_f32(p_pb2, D);
            const std::pair<int64_t, int64_t> f18 = fp8 ? pack8(p_f1w, 4 * D, D) : std::pair<int64_t, int64_t>{0, 0};
            const int64_t w_f1 = fp8 ? f18.first : pack_bf16(p_f1w, 4 * D, D), s_f1 = f18.second, b_f1 = pack_f32(p_f1b, 4 * D);
            const std::pair<int64_t, int64_t> f28 = fp8 ? pack8(p_f2w, D, 4 * D) : std::pair<int64_t, int64_t>{0, 0};
            const int64_t w_f2 = fp8 ? f28.first : pack_bf16(p_f2w, D, 4 * D), s_f2 = f28.second, b_f2 = pack_f32(p_f2b, D);
            const int m0 = i * 6 * D;                                // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
            pack_bf16_at(p_mw, 6 * D, D, w_mod + (int64_t)m0 * D * 2);
            pack_f32_at(p_mb, 6 * D, b_mod + (int64_t)m0 * 4);

            op(fp8 ? OpFn(ln_mod8(m0, m0 + D)) : OpFn(ln_mod(m0, m0 + D)));
            op([=](const Ctx& c) {
                GemmArgs g = gemm_defaults();                       // q | k (| v)
                g.M = c.B * T; g.N = QL; g.bias_n = c.w<float>(b_qk); g.c = c.at<bf16>(qk); g.c_ld = QL;      // (bf16 out in both modes: the attention stays bf16)
                if (fp8) {
                    g.a0 = reinterpret_cast<const bf16*>(c.at<uint8_t>(h8)); g.a0_ld = D; g.a0_C = D; g.b = reinterpret_cast<const bf16*>(c.w<uint8_t>(w_qk)); g.b_ld = D;
                    g.deq_m = c.at<float>(sx); g.deq_n = c.w<float>(s_qk);
                    launch_gemm_fp8(g, c.stream);
                } else {
                    g.a0 = c.at<bf16>(h); g.a0_ld = D; g.a0_C = D; g.b = c.w<bf16>(w_qk); g.b_ld = D;
                    launch_gemm(g, c.stream);
                }
                if (fused_attn && T != 256) {                       // keys streamed through LDS (dit_flash.h)
                    const bf16* qkv = c.at<bf16>(qk);
                    launch_dit_flash(qkv, qkv + D, qkv + 2 * D, 3 * D, c.at<bf16>(o), D, c.B, H, T, hd, c.stream);
                } else if (fused_attn) {                            // softmax(q k^T / sqrt(hd)) v, all heads, one launch
                    if (hd <= 64) launch_attn<2, 4>(c.at<bf16>(qk), c.at<bf16>(o), c.B, D, H, hd, c.stream);
                    else if (hd <= 80) launch_attn<3, 5>(c.at<bf16>(qk), c.at<bf16>(o), c.B, D, H, hd, c.stream);
                    else launch_attn<3, 6>(c.at<bf16>(qk), c.at<bf16>(o), c.B, D, H, hd, c.stream);
                } else {
                g = gemm_defaults();                                // V^T[b] = Wv h[b]^T + bv  ([D][T] per sample)
                g.a0_ld = D; g.a0_C = D; g.a_bs = 0; g.M = D; g.N = T; g.b_ld = D; g.b_bs = (int64_t)T * D; g.bias_m = c.w<float>(b_v);
                g.c = c.at<bf16>(vT); g.c_ld = T; g.c_bs = (int64_t)D * T; g.batch = c.B;
                if (fp8) {                                          // the weights as the row operand: their scales per row, the tokens' per column
                    g.a0 = reinterpret_cast<const bf16*>(c.w<uint8_t>(w_v)); g.b = reinterpret_cast<const bf16*>(c.at<uint8_t>(h8));
                    g.deq_m = c.w<float>(s_v); g.deq_m_bs = 0; g.deq_n = c.at<float>(sx); g.deq_n_bs = T;
                    launch_gemm_fp8(g, c.stream);
                } else {
                    g.a0 = c.w<bf16>(w_v); g.b = c.at<bf16>(h);
                    launch_gemm(g, c.stream);
                }
                for (int hh = 0; hh < H; ++hh) {                    // S[b][hh] = q k^T / sqrt(hd)
                    g = gemm_defaults();
                    g.a0 = c.at<bf16>(qk) + hh * hd; g.a0_ld = 2 * D; g.a0_C = hd; g.a_bs = (int64_t)T * 2 * D; g.M = T; g.N = T;
                    g.b = c.at<bf16>(qk) + D + hh * hd; g.b_ld = 2 * D; g.b_bs = (int64_t)T * 2 * D;
                    g.scale = 1.0f / sqrtf((float)hd);
                    g.c = c.at<float>(S) + (int64_t)hh * T * T; g.c_ld = T; g.c_bs = (int64_t)H * T * T; g.c_mode = OUT_F32; g.batch = c.B;
                    launch_gemm(g, c.stream);
                }
                const int64_t rows = (int64_t)c.B * H * T;
                if (T == 256) hipLaunchKernelGGL(k_softmax_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, c.stream, c.at<float>(S), c.at<bf16>(P), T, rows);
                else hipLaunchKernelGGL(k_softmax_rows_1k, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, c.stream, c.at<float>(S), c.at<bf16>(P), T, rows);
                for (int hh = 0; hh < H; ++hh) {                    // o[b][:, hh*hd : (hh+1)*hd] = P V
                    g = gemm_defaults();
                    g.a0 = c.at<bf16>(P) + (int64_t)hh * T * T; g.a0_ld = T; g.a0_C = T; g.a_bs = (int64_t)H * T * T; g.M = T; g.N = hd;
                    g.b = c.at<bf16>(vT) + (int64_t)hh * hd * T; g.b_ld = T; g.b_bs = (int64_t)D * T;
                    g.c = c.at<bf16>(o) + hh * hd; g.c_ld = D; g.c_bs = (int64_t)T * D; g.batch = c.B;
                    launch_gemm(g, c.stream);
                }
                }
                g = gemm_defaults();                                // x += gate_msa * (o Wproj + b)
                g.a0 = c.at<bf16>(o); g.a0_ld = D; g.a0_C = D; g.M = c.B * T; g.N = D; g.b = c.w<bf16>(w_pr); g.b_ld = D;
                g.bias_n = c.w<float>(b_pr); g.gate = c.at<float>(mod) + m0 + 2 * D; g.gate_ld = nmod; g.log_rows_per_sample = log_T;
                g.resid_f32 = c.at<float>(x); g.resid_f32_ld = D; g.c = c.at<float>(x); g.c_ld = D; g.c_mode = OUT_F32; g.stream_f16 = s16;
                g.stream_guard = c.site(1 + 2 * i);
                launch_gemm(g, c.stream);
            });
            op(fp8 ? OpFn(ln_mod8(m0 + 3 * D, m0 + 4 * D)) : OpFn(ln_mod(m0 + 3 * D, m0 + 4 * D)));
            if (fp8) op([=](const Ctx& c) {
                const int M = c.B * T;
                GemmArgs g = gemm_defaults();                       // GELU_tanh(fc1) -> e4m3 + a scale per 32 columns: fc2's operand
                g.a0 = reinterpret_cast<const bf16*>(c.at<uint8_t>(h8)); g.a0_ld = D; g.a0_C = D; g.M = M; g.N = 4 * D;
                g.b = reinterpret_cast<const bf16*>(c.w<uint8_t>(w_f1)); g.b_ld = D; g.deq_m = c.at<float>(sx); g.deq_n = c.w<float>(s_f1);
                g.bias_n = c.w<float>(b_f1); g.act = ACT_GELU_TANH; g.c = c.at<uint8_t>(f8); g.c_ld = 4 * D; g.c_mode = OUT_FP8_MX;
                g.c_mx = c.at<uint8_t>(fmx); g.c_mx_ld = M;
                launch_gemm_fp8(g, c.stream);
                g = gemm_defaults();                                // x += gate_mlp * (f8 W2^T + b)
                g.a0 = reinterpret_cast<const bf16*>(c.at<uint8_t>(f8)); g.a0_ld = 4 * D; g.a0_C = 4 * D; g.M = M; g.N = D;
                g.a_mx = c.at<uint8_t>(fmx); g.a_mx_ld = M;
                g.b = reinterpret_cast<const bf16*>(c.w<uint8_t>(w_f2)); g.b_ld = 4 * D; g.deq_n = c.w<float>(s_f2);
                g.bias_n = c.w<float>(b_f2); g.gate = c.at<float>(mod) + m0 + 5 * D; g.gate_ld = nmod; g.log_rows_per_sample = log_T;
                g.resid_f32 = c.at<float>(x); g.resid_f32_ld = D; g.c = c.at<float>(x); g.c_ld = D; g.c_mode = OUT_F32; g.stream_f16 = s16;
                g.stream_guard = c.site(2 + 2 * i);
                launch_gemm_fp8(g, c.stream);
            });
            else op([=](const Ctx& c) {
                GemmArgs g = gemm_defaults();                       // GELU_tanh(fc1)
                g.a0 = c.at<bf16>(h); g.a0_ld = D; g.a0_C = D; g.M = c.B * T; g.N = 4 * D; g.b = c.w<bf16>(w_f1); g.b_ld = D;
                g.bias_n = c.w<float>(b_f1); g.act = ACT_GELU_TANH; g.c = c.at<bf16>(f); g.c_ld = 4 * D;
                launch_gemm(g, c.stream);
                g = gemm_defaults();                                // x += gate_mlp * fc2
                g.a0 = c.at<bf16>(f); g.a0_ld = 4 * D; g.a0_C = 4 * D; g.M = c.B * T; g.N = D; g.b = c.w<bf16>(w_f2); g.b_ld = 4 * D;
                g.bias_n = c.w<float>(b_f2); g.gate = c.at<float>(mod) + m0 + 5 * D; g.gate_ld = nmod; g.log_rows_per_sample = log_T;
                g.resid_f32 = c.at<float>(x); g.resid_f32_ld = D; g.c = c.at<float>(x); g.c_ld = D; g.c_mode = OUT_F32; g.stream_f16 = s16;
                g.splitk_ws = c.at<float>(skw); g.splitk_max = SK_MAX;
                g.stream_guard = c.site(2 + 2 * i);
                launch_gemm(g, c.stream);
            });
        }
        // ---- final layer
        const int64_t p_fw = take((int64_t)32 * D), p_fb = take(32), p_fmw = take((int64_t)2 * D * D), p_fmb = take(2 * D);
        const int64_t w_f = pack_bf16(p_fw, 32, D), b_f = pack_f32(p_fb, 32);
        const int mf = 6 * depth * D;
        pack_bf16_at(p_fmw, 2 * D, D, w_mod + (int64_t)mf * D * 2);
        pack_f32_at(p_fmb, 2 * D, b_mod + (int64_t)mf * 4);
        op(ln_mod(mf, mf + D));
        op([=](const Ctx& c) {
            GemmArgs g = gemm_defaults();
            g.a0 = c.at<bf16>(h); g.a0_ld = D; g.a0_C = D; g.M = c.B * T; g.N = 32; g.b = c.w<bf16>(w_f); g.b_ld = D;
            g.bias_n = c.w<float>(b_f); g.c = c.at<float>(tok); g.c_ld = 32; g.c_mode = OUT_F32;
            launch_gemm(g, c.stream);
            const int64_t tot = (int64_t)c.B * 8 * (2 * gs) * (2 * gs);
            hipLaunchKernelGGL(k_unpatchify, dim3(grid1d(tot, 256, 1 << 30)), dim3(256), 0, c.stream, c.at<float>(tok), c.out, 8, gs, tot);
        });
        finish();
    }
};

}  // namespace

extern "C" {

int natinf_dit_create(natinf_dit_t* out, int depth, int hidden, int heads, int flags) {
    return natinf_dit_create_sized(out, depth, hidden, heads, 32, flags);
}
int natinf_dit_create_sized(natinf_dit_t* out, int depth, int hidden, int heads, int input_size, int flags) {
    if (!out || (flags & ~(NATINF_DIT_UNFUSED_ATTENTION | NATINF_DIT_FP8 | NATINF_DIT_STREAM_GUARD)) || ((flags & NATINF_DIT_FP8) && hidden % 128) || depth <= 0 || hidden <= 0 || heads <= 0 || hidden % 64 || hidden % heads || (hidden / heads) % 8 || hidden > 1536)
        return NATINF_EINVAL;
    if (input_size != 32 && input_size != 64) return NATINF_EINVAL;
    natinf_dit* e = new natinf_dit();
    e->depth = depth; e->D = hidden; e->heads = heads; e->hd = hidden / heads;
    e->input_size = input_size; e->T = (input_size / 2) * (input_size / 2);
    e->unfused_attention = (flags & NATINF_DIT_UNFUSED_ATTENTION) != 0;
    e->fp8 = (flags & NATINF_DIT_FP8) != 0;
    e->stream16 = g_dit_stream16 != 0;
    e->guard_sites = (flags & NATINF_DIT_STREAM_GUARD) ? 1 + 2 * depth : 0;
    DitBuilder b(*e);
    b.build();
    *out = e;
    return NATINF_OK;
}
int natinf_set_dit_stream16(int on) { g_dit_stream16 = on < 0 ? DIT_STREAM16_DEFAULT : (on != 0); return NATINF_OK; }
int natinf_dit_input_size(natinf_dit_t h) { return h ? h->input_size : NATINF_EINVAL; }
int natinf_dit_destroy(natinf_dit_t h) { if (!h) return NATINF_EINVAL; delete h; return NATINF_OK; }
int64_t natinf_dit_param_count(natinf_dit_t h) { return h ? h->n_params : NATINF_EINVAL; }
int64_t natinf_dit_packed_bytes(natinf_dit_t h) { return h ? h->packed_bytes : NATINF_EINVAL; }
int64_t natinf_dit_workspace_bytes(natinf_dit_t h, int max_batch) { return h && max_batch > 0 ? h->workspace_bytes(max_batch) : NATINF_EINVAL; }
int natinf_dit_stream_sites(natinf_dit_t h) { return h && h->guard_sites ? h->guard_sites : NATINF_EINVAL; }
int natinf_dit_stream_status_reset(natinf_dit_t h, void* workspace, natinf_stream_t stream) { return h ? h->status_reset(workspace, (hipStream_t)stream) : NATINF_EINVAL; }
int natinf_dit_stream_status(natinf_dit_t h, const void* workspace, uint32_t* out_dev, natinf_stream_t stream) { return h ? h->status_read(workspace, out_dev, (hipStream_t)stream) : NATINF_EINVAL; }

int natinf_dit_load(natinf_dit_t h, const float* params_f32, int64_t n_params, void* packed, int64_t packed_bytes, natinf_stream_t stream) {
    return h ? h->load(params_f32, n_params, packed, packed_bytes, (hipStream_t)stream) : NATINF_EINVAL;
}

int natinf_dit_forward(natinf_dit_t h, const float* z, const float* t, const int32_t* y, float* out, int B, void* workspace,
                       int64_t workspace_bytes, natinf_stream_t stream) {
    if (!h || !y) return NATINF_EINVAL;
    h->y = y;
    return h->run(z, t, out, B, workspace, workspace_bytes, (hipStream_t)stream);
}

int natinf_dit_attention_bf16(const void* q, const void* k, const void* v, int ld, void* o, int ld_o, int B, int T, int H, int hd, int flags,
                              natinf_stream_t stream) {
    if (!q || !k || !v || !o || B <= 0 || H <= 0 || hd < 8 || hd > 96 || hd % 8 || ld % 8 || ld < H * hd || ld_o % 4 || ld_o < H * hd) return NATINF_EINVAL;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) % 16 || reinterpret_cast<uintptr_t>(o) % 8) return NATINF_EINVAL;
    if (flags & ~NATINF_DIT_ATTN_RESIDENT) return NATINF_EINVAL;
    const bool resident = (flags & NATINF_DIT_ATTN_RESIDENT) != 0;
    if (resident ? T != 256 : (T < 256 || T > 4096 || T % 128)) return NATINF_EINVAL;
    if (!configure_gemm_kernels()) return NATINF_ENODEV;
    if (resident) {                                      // k_attn_fused addresses k as q + k_off
        const int64_t k_off = (int64_t)(reinterpret_cast<intptr_t>(k) - reinterpret_cast<intptr_t>(q)) / 2;
        if (k_off > INT32_MAX || k_off < INT32_MIN) return NATINF_EINVAL;
        const bf16* qb = (const bf16*)q;
        const bf16* vb = (const bf16*)v;
        bf16* ob = (bf16*)o;
        const float sc = 1.0f / sqrtf((float)hd);
        const hipStream_t s = (hipStream_t)stream;
        auto run = [&](auto kern, int lds) { hipLaunchKernelGGL(kern, dim3((unsigned)(B * H)), dim3(512), lds, s, qb, ld, (int)k_off, vb, ob, ld_o, H, hd, sc); };
        if (hd <= 64) run(&k_attn_fused<2, 4, false, true>, AttnCfg<2, 4>::LDS_BYTES);
        else if (hd <= 80) run(&k_attn_fused<3, 5, false, true>, AttnCfg<3, 5>::LDS_BYTES);
        else run(&k_attn_fused<3, 6, false, true>, AttnCfg<3, 6>::LDS_BYTES);
    } else {
        launch_dit_flash((const bf16*)q, (const bf16*)k, (const bf16*)v, ld, (bf16*)o, ld_o, B, H, T, hd, (hipStream_t)stream);
    }
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}

}  // extern "C"
