// transformer_rows.h -- the row and glue kernels the transformer engines (DiT, SD3 MMDiT; dit_engine.inc, mmdit_engine.inc) share: the patch embedding (plain and
// guarded: one template, its guarded instances live in stream_guard.hip), the LayerNorm-modulate family with its launcher, the conditioning / unpatchify / cast glue
// and the 1,024-key row softmax.  Like the other kernel headers it may be included into an anonymous namespace (stream_guard.hip): it defines nothing with external
// linkage, and the LayerNorm-modulate kernels and their launcher are templates, so a unit that launches none of them carries none of them.
// Tested alone against fp64: the LayerNorm-modulate family and k_softmax_rows_1k by tests/test_gpu_row_kernels.py (cases: tests/row_kernel_cases.py); k_patch_embed (all four
// instances), k_dit_time_freq, k_dit_cond, k_unpatchify, k_f32_to_bf16 and k_silu_bf16 by tests/test_gpu_glue_kernels.py (cases, radii and what each catches:
// tests/glue_kernel_cases.py, tests/test_glue_kernels_host.py), through the natinf_debug_* entries of dit_engine.inc and the launchers of transformer_plan.h.
#pragma once
#include "gemm_dma.h"

namespace ncsn {

// x[b*T + t][d] = sum_k W[d][k] * patch(b, t)[k] + bias[d] + pos[t][d];  k = (c, pi, qi) as Conv2d(p, stride p) flattens
// z [B][C][2g][2g], patch 2, g x g tokens per sample; Wt = the conv weight TRANSPOSED to [C*4][D].  A block owns 256
// output channels of PE_TOK consecutive tokens: the 4C patch values of those tokens are staged in LDS once, every weight
// is read once per block (coalesced) and reused for all PE_TOK tokens from a register.
// GUARD: the guarded form (NATINF_DIT_STREAM_GUARD / NATINF_MMDIT_STREAM_GUARD: site 0 of the status block; ncsnpp_kernels.h states the guard): the same sums in the same
// order, every value through stream_guard_value before it is stored.  D % 64 == 0, so a wave is past D as a whole or not at all: the waves that stay commit with 64 lanes.
constexpr int PE_TOK = 16;
template <bool XH, bool GUARD>                                            // XH: x is written as IEEE half (the engines' 16-bit residual stream); guard: read by GUARD only
__global__ __launch_bounds__(256) void k_patch_embed(const float* __restrict__ z, const float* __restrict__ Wt,
                                                     const float* __restrict__ bias, const float* __restrict__ pos,
                                                     float* __restrict__ x, int C, int g, int D, int64_t rows, uint32_t* __restrict__ guard)
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
    [[maybe_unused]] StreamGuardAcc ga;
#pragma unroll
    for (int tk = 0; tk < PE_TOK; ++tk) {
        const int64_t row = row0 + tk;
        if (row < rows) {
            float v = acc[tk] + pos[(row % T) * D + d];
            if constexpr (GUARD) v = stream_guard_value<XH>(ga, v);
            if constexpr (XH) reinterpret_cast<_Float16*>(x)[row * D + d] = (_Float16)v; else x[row * D + d] = v;
        }
    }
    if constexpr (GUARD) stream_guard_commit(ga, guard);
}
template <bool GUARD>
inline void launch_patch_embed_as(const float* z, const float* Wt, const float* bias, const float* pos, float* x, int C, int g, int D, int64_t rows, bool x_f16, uint32_t* guard,
                                  hipStream_t s)
{
    const dim3 grid((unsigned)((D + 255) / 256), (unsigned)((rows + PE_TOK - 1) / PE_TOK));
    if (x_f16) hipLaunchKernelGGL((k_patch_embed<true, GUARD>), grid, dim3(256), 0, s, z, Wt, bias, pos, x, C, g, D, rows, guard);
    else hipLaunchKernelGGL((k_patch_embed<false, GUARD>), grid, dim3(256), 0, s, z, Wt, bias, pos, x, C, g, D, rows, guard);
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

// ---- h = LayerNorm(x) * (1 + scale[b]) + shift[b]  (no affine, eps 1e-6); one wave per token row, fp32 statistics.  Three load forms (scalar, four columns, eight
// columns of a half stream), each one kernel template over what becomes of the modulated row -- the output policy Out; the kernels are the same line for line up to
// the modulation, and an instance compiles to what the separate kernel compiled to (plain pointer arguments: passed inside a struct, every instance came out different).
struct RowsBf16 { typedef bf16 T; static constexpr bool FP8 = false; };         // h: bf16 rows; row_scale is not read (null)
// h: fp8 e4m3 rows with one scale per row in row_scale (k_gemm_fp8's A operand, gemm_fp8.h): q = round(v / s), s = max|v| / 448 (the e4m3 maximum; values are
// clamped, v_cvt_pk_fp8_f32 does not saturate)
struct RowsFp8 { typedef uint8_t T; static constexpr bool FP8 = true; };

__device__ __forceinline__ float ln_mod(float v, float mean, float rstd, float g, float t) { return (v - mean) * rstd * (1.0f + g) + t; }
// the row's e4m3 scale from the lanes' maxima
__device__ __forceinline__ float fp8_row_scale(float amax)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    return amax > 0.f ? amax / 448.0f : 1.0f;
}

// The scalar form, any D % 64 == 0 up to 1,536 (fp8 rows: D % 128 == 0).  x_f16: the residual stream is IEEE half -- the engines' 16-bit stream, natinf_set_dit_stream16 /
// natinf_set_mmdit_stream16 -- read through the same pointer.  The two policies own DIFFERENT columns per lane, so they add the row statistics in different orders
// (tests/row_kernel_cases.py restates both): bf16 rows lane + 64 i; fp8 rows the adjacent pair 2 lane, 2 lane + 1 of every 128 (one 8-byte load, one 2-byte store).
template <class Out>
__global__ __launch_bounds__(256) void k_ln_modulate(const float* __restrict__ x, const float* __restrict__ shift,
                                                     const float* __restrict__ scale, int mod_ld, typename Out::T* __restrict__ h, float* __restrict__ row_scale,
                                                     int D, int64_t rows, int rows_per_sample, int x_f16)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * D;
    const _Float16* xh = reinterpret_cast<const _Float16*>(x) + row * D;
    float v[24];                                                    // D <= 1536
    const int n = D >> 6;
    float s = 0.f;
    if constexpr (Out::FP8) {
        for (int i = 0; i < n; i += 2) {
            float2 u;
            if (x_f16) { u.x = (float)xh[64 * i + 2 * lane]; u.y = (float)xh[64 * i + 2 * lane + 1]; }
            else u = *reinterpret_cast<const float2*>(xr + 64 * i + 2 * lane);
            v[i] = u.x; v[i + 1] = u.y; s += u.x + u.y;
        }
    } else {
        for (int i = 0; i < n; ++i) { v[i] = x_f16 ? (float)xh[lane + 64 * i] : xr[lane + 64 * i]; s += v[i]; }
    }
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
    if constexpr (Out::FP8) {
        float amax = 0.f;
        for (int i = 0; i < n; i += 2) {
            const int d = 64 * i + 2 * lane;
            v[i] = ln_mod(v[i], mean, rstd, sc[d], sh[d]);
            v[i + 1] = ln_mod(v[i + 1], mean, rstd, sc[d + 1], sh[d + 1]);
            amax = fmaxf(amax, fmaxf(fabsf(v[i]), fabsf(v[i + 1])));
        }
        const float qs = fp8_row_scale(amax), inv = 1.0f / qs;
        if (lane == 0) row_scale[row] = qs;
        for (int i = 0; i < n; i += 2) {
            const float a = fminf(fmaxf(v[i] * inv, -448.f), 448.f), c = fminf(fmaxf(v[i + 1] * inv, -448.f), 448.f);
            const int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, c, 0, false);
            *reinterpret_cast<uint16_t*>(h + row * D + 64 * i + 2 * lane) = (uint16_t)(w & 0xffff);
        }
    } else {
        for (int i = 0; i < n; ++i) {
            const int d = lane + 64 * i;
            h[row * D + d] = (bf16)ln_mod(v[i], mean, rstd, sc[d], sh[d]);
        }
    }
}
// The same for D = NC * 256 + REM (SD3: 1536): a lane owns four consecutive columns per 256-column chunk -- 16-byte loads of x, scale and shift, 8-byte stores of bf16
// (4-byte stores of e4m3), everything unrolled.  The scalar form above moved 300 MB per SD3 image-stream launch at 2.4 TB/s (8 % of the forward,
// profiles/r02/sd3_kernel_stats.csv): one 4-byte load per lane and instruction, three loads per element.
// REM % 4 == 0: the last, partial chunk is owned by lanes 0 .. REM / 4 - 1 (DiT-XL/2: 1152 = 4 * 256 + 128)
// XH: x is IEEE half (8-byte loads of four columns; the statistics and the modulation stay fp32)
template <int NC, int REM, bool XH, class Out>
__global__ __launch_bounds__(256) void k_ln_modulate_v4(const float* __restrict__ x, const float* __restrict__ shift,
                                                        const float* __restrict__ scale, int mod_ld, typename Out::T* __restrict__ h, float* __restrict__ row_scale,
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
    if constexpr (Out::FP8) {
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if (i < NC || tail) {
                const float4 g = sc[64 * i], t = sh[64 * i];
                v[i].x = ln_mod(v[i].x, mean, rstd, g.x, t.x); v[i].y = ln_mod(v[i].y, mean, rstd, g.y, t.y);
                v[i].z = ln_mod(v[i].z, mean, rstd, g.z, t.z); v[i].w = ln_mod(v[i].w, mean, rstd, g.w, t.w);
                amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v[i].x), fabsf(v[i].y)), fmaxf(fabsf(v[i].z), fabsf(v[i].w))));
            }
        }
        const float qs = fp8_row_scale(amax), inv = 1.0f / qs;
        if (lane == 0) row_scale[row] = qs;
        unsigned* out = reinterpret_cast<unsigned*>(h + row * D) + lane;
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (i < NC || tail) out[64 * i] = pack_fp8x4(v[i].x * inv, v[i].y * inv, v[i].z * inv, v[i].w * inv);
    } else {
        uint2* out = reinterpret_cast<uint2*>(h + row * D) + lane;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if (i < NC || tail) {
                const float4 g = sc[64 * i], t = sh[64 * i];
                bf16x4_t o;
                o[0] = (bf16)ln_mod(v[i].x, mean, rstd, g.x, t.x); o[1] = (bf16)ln_mod(v[i].y, mean, rstd, g.y, t.y);
                o[2] = (bf16)ln_mod(v[i].z, mean, rstd, g.z, t.z); o[3] = (bf16)ln_mod(v[i].w, mean, rstd, g.w, t.w);
                out[64 * i] = __builtin_bit_cast(uint2, o);
            }
        }
    }
}
// The half stream in 16-byte accesses (D = NC8 * 512; SD3: 1536): a lane owns EIGHT consecutive columns per 512-column chunk -- one 16-byte load of x, two of scale and of
// shift, one 16-byte store of bf16 (one 8-byte store of e4m3).  bf16 rows: alone it takes 35 us per SD3 image-stream launch (200 MB: 5.7 TB/s); inside a forward its mean
// is ~50 us like the four-column form's (51.6 us: profiles/r06/sd3_kernel_stats.csv) -- the text stream's GEMMs run beside it on their own HIP stream (min 35, max 79 us
// over a forward's 96 launches).  fp8 rows: 32 us alone; ~49 us mean inside a forward, beside the text stream's launches, like the four-column form.
// Same arithmetic per element; the row statistics are summed in another order (fp32: last-bit differences).
template <int NC8, class Out>
__global__ __launch_bounds__(256) void k_ln_modulate_h8(const float* __restrict__ x, const float* __restrict__ shift, const float* __restrict__ scale, int mod_ld,
                                                        typename Out::T* __restrict__ h, float* __restrict__ row_scale, int64_t rows, int rows_per_sample)
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
    if constexpr (Out::FP8) {
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < NC8; ++i) {
            const float4 g0 = sc[128 * i], g1 = sc[128 * i + 1], t0 = sh[128 * i], t1 = sh[128 * i + 1];
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, tt[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[i][e] = ln_mod(v[i][e], mean, rstd, gg[e], tt[e]); amax = fmaxf(amax, fabsf(v[i][e])); }
        }
        const float qs = fp8_row_scale(amax), inv = 1.0f / qs;
        if (lane == 0) row_scale[row] = qs;
        uint2* out = reinterpret_cast<uint2*>(h + row * D) + lane;
#pragma unroll
        for (int i = 0; i < NC8; ++i)
            out[64 * i] = make_uint2(pack_fp8x4(v[i][0] * inv, v[i][1] * inv, v[i][2] * inv, v[i][3] * inv), pack_fp8x4(v[i][4] * inv, v[i][5] * inv, v[i][6] * inv, v[i][7] * inv));
    } else {
        uint4* out = reinterpret_cast<uint4*>(h + row * D) + lane;
#pragma unroll
        for (int i = 0; i < NC8; ++i) {
            const float4 g0 = sc[128 * i], g1 = sc[128 * i + 1], t0 = sh[128 * i], t1 = sh[128 * i + 1];
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, tt[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
            bf16x8_ln o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16)ln_mod(v[i][e], mean, rstd, gg[e], tt[e]);
            out[64 * i] = __builtin_bit_cast(uint4, o);
        }
    }
}
// One dispatch table on (D, alignment of the modulation rows, x_f16) for both policies.  Returns the form it launched -- 0 scalar, 1 four-column, 2 eight-column -- for
// natinf_debug_ln_modulate (tests/test_gpu_row_kernels.py); the engines ignore it.
template <class Out>
inline int launch_ln_modulate(const float* x, const float* shift, const float* scale, int mod_ld, typename Out::T* h, float* row_scale, int D, int64_t rows, int rows_per_sample, hipStream_t s,
                              bool x_f16 = false)
{
    const dim3 grid((unsigned)((rows + 3) / 4));
    const bool al = mod_ld % 4 == 0 && (reinterpret_cast<uintptr_t>(shift) | reinterpret_cast<uintptr_t>(scale)) % 16 == 0;
    auto go = [&](auto kern, int form) { hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, x, shift, scale, mod_ld, h, row_scale, rows, rows_per_sample); return form; };
    if (al && x_f16) {                                                  // the engines' 16-bit residual stream
        if (D == 1536) return go(&k_ln_modulate_h8<3, Out>, 2);
        if (D == 256) return go(&k_ln_modulate_v4<1, 0, true, Out>, 1);
        if (D == 1152) return go(&k_ln_modulate_v4<4, 128, true, Out>, 1);      // DiT-XL/2
    } else if (al) {
        if (D == 1536) return go(&k_ln_modulate_v4<6, 0, false, Out>, 1);
        if (D == 256) return go(&k_ln_modulate_v4<1, 0, false, Out>, 1);
        if (D == 1152) return go(&k_ln_modulate_v4<4, 128, false, Out>, 1);     // DiT-XL/2
    }
    hipLaunchKernelGGL(k_ln_modulate<Out>, grid, dim3(256), 0, s, x, shift, scale, mod_ld, h, row_scale, D, rows, rows_per_sample, (int)x_f16);
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
