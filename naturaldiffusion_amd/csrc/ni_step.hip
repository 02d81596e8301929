// ni_step.hip -- the Natural Inference recurrence as fused gfx950 streaming kernels.
//
// One launch per sampling step does everything the reference does between two denoiser
// calls: model output -> x0_hat, append to the history slab, coefficient-row weighted sum
// over the history (+ noise mixing), cast.  The kernels are HBM-bound (0.1-0.25 flop/B), so
// the design rules are the streaming ones: 16-byte vector accesses, one coalesced stream per
// history row ([slot][E] slab), coefficients through the scalar cache (wave-uniform s_load, no
// LDS needed), unrolled term loop so several row loads are in flight, <= 2048 resident blocks
// with a grid-stride loop.
//
// Arithmetic contract (include/natinf.h): operand types and operation ORDER of the reference,
// one IEEE rounding per reference operation.  The file is compiled -ffp-contract=off and the
// pragma below repeats it, so no mul+add pair is ever fused.
//
// Every expression of that contract is written ONCE, as a __device__ __forceinline__ piece that keeps
// the named fp32 / fp64 temporaries which fix its roundings; a kernel is a short composition of pieces,
// so a kernel with in-kernel noise cannot drift from its slab twin (DESIGN.md section 3 lists them).  Whole step bodies are pieces too: a new conditioning
// is a new piece plus a thin __global__ function, never a copied body.  The kernels' listings rest on this: kernel names, template parameters and __global__
// parameter lists stay; pointers stay individual __restrict__ parameters, never bundled into by-value structs (after the store of hist[k] that keeps the
// coefficient rows on wave-uniform scalar loads; ProjGeom and mat3 hold scalars only); kernels are not merged into bool-templated ones; every empty-asm pin
// (hmulf, the Philox key of k_stepfix_f64 / k_stepproject_f64, ld_whole, color_blend's planes) stays where it is relative to its loop; the Philox kernels
// keep one quad per thread.  The loop of k_stepfix_f64 / k_stepproject_f64 that fills the LDS planes stays in them: as a piece it changed their addressing.
//
// Reference lines replaced: src/CIFAR10NaturalInference.py:219-238,299-304;
// src/ValidateNaturalInference.py:193,198-204,355,362-366; src/SD3NaturalInference.py:61-69,
// 117-129,157-168,209,215-219; deps/score_sde_pytorch/models/utils.py:157; deps/dpm_solver_pytorch.py:416-425 (the x0 correction: its
// quantile interpolation is the one __builtin_fma of this file).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cfloat>
#include <cmath>
#include <mutex>
#include "natinf.h"
#include "natinf_vae.h"
#include "posterior_ws.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;            // 256 CUs x 8 blocks: enough to fill the chip, grid-stride the rest

inline int grid_for(int64_t nvec) {
    int64_t g = (nvec + kBlock - 1) / kBlock;
    return (int)(g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g));
}

// grid-stride loop: for (v = first_vec(); v < nvec; v += vec_stride())
__device__ __forceinline__ int64_t first_vec() { return (int64_t)blockIdx.x * kBlock + threadIdx.x; }
__device__ __forceinline__ int64_t vec_stride() { return (int64_t)gridDim.x * kBlock; }

struct alignas(16) d2 { double x, y; };
typedef _Float16 h16;
struct alignas(16) h8 { h16 v[8]; };

// fp32 product of an fp32 scalar and an fp16 value, rounded to fp32 and THEN to fp16 (what eager
// PyTorch does).  The empty asm pins the fp32 product in a VGPR so the backend cannot select
// v_fma_mixlo_f16 (x*y + (+0)), whose +0 addend would turn a -0 product into +0.
__device__ __forceinline__ h16 hmulf(float s, h16 a) {
    float p = s * (float)a;
    asm("" : "+v"(p));
    return (h16)p;
}
__device__ __forceinline__ h16 hadd(h16 a, h16 b) { return (h16)((float)a + (float)b); }
__device__ __forceinline__ h16 hsub(h16 a, h16 b) { return (h16)((float)a - (float)b); }

__device__ __forceinline__ h8 h8_zero() {
    h8 z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z.v[i] = (h16)0.0f;
    return z;
}

// acc <- fp16 chain over the sparse row; hand-unrolled by 4 so four row loads are in flight
// (the asm pin in hmulf keeps the compiler from unrolling the loop itself).
__device__ __forceinline__ void chain_terms(h8& acc, const h16* __restrict__ hist, const int32_t* __restrict__ idx,
                                            const float* __restrict__ val, int n_terms, int64_t v, int64_t E)
{
    int t = 0;
    for (; t + 4 <= n_terms; t += 4) {
        const float c0 = val[t], c1 = val[t + 1], c2 = val[t + 2], c3 = val[t + 3];
        const h8 h0 = reinterpret_cast<const h8*>(hist + (int64_t)idx[t] * E)[v];
        const h8 h1 = reinterpret_cast<const h8*>(hist + (int64_t)idx[t + 1] * E)[v];
        const h8 h2 = reinterpret_cast<const h8*>(hist + (int64_t)idx[t + 2] * E)[v];
        const h8 h3 = reinterpret_cast<const h8*>(hist + (int64_t)idx[t + 3] * E)[v];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            acc.v[i] = hadd(acc.v[i], hmulf(c0, h0.v[i]));
            acc.v[i] = hadd(acc.v[i], hmulf(c1, h1.v[i]));
            acc.v[i] = hadd(acc.v[i], hmulf(c2, h2.v[i]));
            acc.v[i] = hadd(acc.v[i], hmulf(c3, h3.v[i]));
        }
    }
    for (; t < n_terms; ++t) {
        const float c = val[t];
        const h8 h = reinterpret_cast<const h8*>(hist + (int64_t)idx[t] * E)[v];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc.v[i] = hadd(acc.v[i], hmulf(c, h.v[i]));
    }
}

// fp16 row mean: fp32 division of the fp16 sum, rounded to fp16
__device__ __forceinline__ h8 mean_of(h8 acc, float w_total) {
    h8 mean;
#pragma unroll
    for (int i = 0; i < 8; ++i) mean.v[i] = (h16)((float)acc.v[i] / w_total);
    return mean;
}

// next flow input sig*noise + oms*mean, every operation rounded to fp16
__device__ __forceinline__ h8 flow_input(h8 nz, h8 m, float sig, float oms) {
    h8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = hadd(hmulf(sig, nz.v[i]), hmulf(oms, m.v[i]));
    return r;
}

// the fused x0 of one 8-vector from the text and null-prompt velocities tv, uv, six fp16 roundings per element whose order is the contract: CFG on
// the velocities, then x - sig*v (kVelocityCfg), or CFG on the two x0 (k_step_f16chain with its launch-wide cfg, x0_cfg_image with the image's)
template <bool kVelocityCfg>
__device__ __forceinline__ h8 x0_cfg(h8 xv, h8 tv, h8 uv, float sig, float cfg) {
    h8 f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (kVelocityCfg) {
            const h16 d = hsub(tv.v[i], uv.v[i]);
            const h16 vv = hadd(uv.v[i], hmulf(cfg, d));
            f.v[i] = hsub(xv.v[i], hmulf(sig, vv));
        } else {
            const h16 x0n = hsub(xv.v[i], hmulf(sig, uv.v[i]));
            const h16 x0t = hsub(xv.v[i], hmulf(sig, tv.v[i]));
            const h16 d = hsub(x0t, x0n);
            f.v[i] = hadd(x0n, hmulf(cfg, d));
        }
    }
    return f;
}

// ---- piece of the SD3 form with per-image guidance (fp16 chain) ----
// the fused x0 of one 8-vector: image img's null-prompt velocity is row uncond_slot[img] of the compacted v_null (quad q of it) and
// its scale cfg_image[img]; a negative slot = an unguided image, f = x - sig*v_text for both flag values (neither v_null nor
// cfg_image[img] is read then).  With a slot it is x0_cfg, the arithmetic of k_step_f16chain for the flag.
// Both per-image values are uniform over the svec consecutive threads of an image: plain vector loads, served by one cache line.
// (k_step_f16chain_guided, k_step_inpaint_f16chain)
template <bool kVelocityCfg>
__device__ __forceinline__ h8 x0_cfg_image(h8 xv, h8 tv, const h8* v_null, const float* cfg_image, const int32_t* uncond_slot,
                                           int64_t img, int64_t q, int64_t svec, float sig)
{
    const int32_t slot = uncond_slot[img];
    if (slot < 0) {
        h8 f;
#pragma unroll
        for (int i = 0; i < 8; ++i) f.v[i] = hsub(xv.v[i], hmulf(sig, tv.v[i]));
        return f;
    }
    const float cfg = cfg_image[img];
    return x0_cfg<kVelocityCfg>(xv, tv, v_null[(int64_t)slot * svec + q], sig, cfg);
}

// f stored as hist[k], then the chain's row mean: chain_terms over the history, the diagonal term c_diag*f, mean_of (the three fp16 step kernels)
__device__ __forceinline__ h8 chain_mean(h8 f, h16* hist, const int32_t* idx, const float* val, int n_terms, float c_diag, float w_total,
                                         int k, int64_t v, int64_t E)
{
    reinterpret_cast<h8*>(hist + (int64_t)k * E)[v] = f;
    h8 acc = h8_zero();
    chain_terms(acc, hist, idx, val, n_terms, v, E);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc.v[i] = hadd(acc.v[i], hmulf(c_diag, f.v[i]));
    return mean_of(acc, w_total);
}

// ---- pieces of the CIFAR10 form (fp64 history) ----
// x0 = ((-out/std) * sigma^2 + x) / alpha: the score in fp32, then three fp64 roundings
__device__ __forceinline__ void x0_score_f64(double (&x0)[4], float4 xv, float4 ov, float stdv, double sigma2, double alpha)
{
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
    const float os[4] = {ov.x, ov.y, ov.z, ov.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float s = (-os[i]) / stdv;                          // score, fp32
        x0[i] = ((double)s * sigma2 + (double)xs[i]) / alpha;     // fp64, three roundings
    }
}

// four fp64 values as quad v of a slab row: two 16-byte stores
__device__ __forceinline__ void st_quad_f64(double* row, int64_t v, const double (&x)[4]) {
    d2* r = reinterpret_cast<d2*>(row) + 2 * v;
    r[0] = d2{x[0], x[1]};
    r[1] = d2{x[2], x[3]};
}

// acc <- acc + h*c, four lanes: one fp64 product, one fp64 sum
__device__ __forceinline__ void acc_f64(double (&acc)[4], double h0, double h1, double h2, double h3, double c) {
    acc[0] = acc[0] + h0 * c; acc[1] = acc[1] + h1 * c;
    acc[2] = acc[2] + h2 * c; acc[3] = acc[3] + h3 * c;
}

__device__ __forceinline__ void wsum_f64(double (&acc)[4], const double* hist, const int32_t* idx, const double* val,
                                         int n_terms, int64_t v, int64_t E)
{
#pragma unroll 4
    for (int t = 0; t < n_terms; ++t) {
        const double c = val[t];
        const d2* hj = reinterpret_cast<const d2*>(hist + (int64_t)idx[t] * E) + 2 * v;
        const d2 a = hj[0], b = hj[1];
        acc_f64(acc, a.x, a.y, b.x, b.y, c);
    }
}

// ---- pieces of the Validate form (fp32 products, fp64 accumulate) ----
// quad q of sample img of the logical [B][sample_elems] tensor inside a [B][sstride] buffer
__device__ __forceinline__ float4 ld_eps(const float* p, int64_t img, int64_t q, int64_t sstride) {
    return *reinterpret_cast<const float4*>(p + img * sstride + 4 * q);
}

// the CFG fuse uncond + cfg*(cond - uncond), four lanes: three fp32 roundings
__device__ __forceinline__ float4 cfg_fuse(float4 ev, float4 uv, float cfg) {
    const float e[4] = {ev.x, ev.y, ev.z, ev.w}, u[4] = {uv.x, uv.y, uv.z, uv.w};
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float d = e[i] - u[i], m = cfg * d; r[i] = u[i] + m; }
    return make_float4(r[0], r[1], r[2], r[3]);
}

// the model's eps: cond, or cfg_fuse with the unconditional row at the same index
__device__ __forceinline__ float4 cfg_eps(const float* cond, const float* uncond, float cfg, int64_t img, int64_t q,
                                          int64_t sstride)
{
    const float4 ev = ld_eps(cond, img, q, sstride);
    return uncond ? cfg_fuse(ev, ld_eps(uncond, img, q, sstride), cfg) : ev;
}

// the model's eps with per-image guidance: image img's unconditional row is uncond[uncond_slot[img]] and its scale
// cfg_image[img]; a negative slot = an unguided image, eps = cond (neither uncond nor cfg_image[img] is read then).
// Both per-image values are uniform over the svec consecutive threads of an image: plain vector loads, served by one cache line.
__device__ __forceinline__ float4 cfg_eps_image(const float* cond, const float* uncond, const float* cfg_image,
                                                const int32_t* uncond_slot, int64_t img, int64_t q, int64_t sstride)
{
    const float4 ev = ld_eps(cond, img, q, sstride);
    const int32_t slot = uncond_slot[img];
    return slot >= 0 ? cfg_fuse(ev, ld_eps(uncond, slot, q, sstride), cfg_image[img]) : ev;
}

// x0 = c1*z - c2*eps: two fp32 products and a subtraction
__device__ __forceinline__ float4 x0_f32prod(float c1, float4 zv, float c2, float4 ev) {
    const float z[4] = {zv.x, zv.y, zv.z, zv.w}, e[4] = {ev.x, ev.y, ev.z, ev.w};
    float x0[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float p = c1 * z[i], q = c2 * e[i]; x0[i] = p - q; }
    return make_float4(x0[0], x0[1], x0[2], x0[3]);
}

// acc <- acc + (double)fp32(h*c), four lanes: history rows, the diagonal term and the noise row all go through here
__device__ __forceinline__ void acc_prod(double (&acc)[4], float4 h, float c) {
    const float p0 = h.x * c, p1 = h.y * c, p2 = h.z * c, p3 = h.w * c;
    acc[0] = acc[0] + (double)p0; acc[1] = acc[1] + (double)p1; acc[2] = acc[2] + (double)p2; acc[3] = acc[3] + (double)p3;
}

__device__ __forceinline__ void wsum_f32prod(double (&acc)[4], const float* hist, const int32_t* idx, const float* val,
                                             int n_terms, int64_t v, int64_t E)
{
#pragma unroll 4
    for (int t = 0; t < n_terms; ++t)
        acc_prod(acc, reinterpret_cast<const float4*>(hist + (int64_t)idx[t] * E)[v], val[t]);
}

// (float)a + (float)b: each fp64 sum is cast once, then one fp32 addition
__device__ __forceinline__ float4 combine(const double (&a)[4], const double (&b)[4]) {
    return make_float4((float)a[0] + (float)b[0], (float)a[1] + (float)b[1],
                       (float)a[2] + (float)b[2], (float)a[3] + (float)b[3]);
}

// the finished x0 quad stored as hist_x0[k], then a <- the signal sum over the history plus the diagonal term (k_step_f32prod, noise_step_f32prod)
__device__ __forceinline__ void signal_sum_f32prod(double (&a)[4], float4 x0, float* hist_x0, const int32_t* idx_c, const float* val_c,
                                                   int n_c, float c_diag, int k, int64_t v, int64_t E)
{
    reinterpret_cast<float4*>(hist_x0 + (int64_t)k * E)[v] = x0;
    wsum_f32prod(a, hist_x0, idx_c, val_c, n_c, v, E);
    acc_prod(a, x0, c_diag);
}

// ------------------------------------------------------------------------------------------
// CIFAR10 form, fp64 history
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_step_f64hist(
    const float4* __restrict__ x_k, const float4* __restrict__ mout, const float4* __restrict__ noise,
    double* __restrict__ hist, float4* __restrict__ x_next,
    const int32_t* __restrict__ idx, const double* __restrict__ val, int n_terms, double c_diag,
    int k, double alpha, double sigma2, float stdv, float b0, int64_t nvec, int64_t E)
{
    for (int64_t v = first_vec(); v < nvec; v += vec_stride()) {
        const float4 nv = noise[v];
        double x0[4], acc[4] = {0.0, 0.0, 0.0, 0.0};
        x0_score_f64(x0, x_k[v], mout[v], stdv, sigma2, alpha);
        st_quad_f64(hist + (int64_t)k * E, v, x0);
        wsum_f64(acc, hist, idx, val, n_terms, v, E);
        acc_f64(acc, x0[0], x0[1], x0[2], x0[3], c_diag);
        x_next[v] = make_float4((float)acc[0] + b0 * nv.x, (float)acc[1] + b0 * nv.y,
                                (float)acc[2] + b0 * nv.z, (float)acc[3] + b0 * nv.w);
    }
}

__global__ __launch_bounds__(kBlock) void k_wsum_f64(
    const double* __restrict__ hist, float4* __restrict__ out,
    const int32_t* __restrict__ idx, const double* __restrict__ val, int n_terms, int64_t nvec, int64_t E)
{
    for (int64_t v = first_vec(); v < nvec; v += vec_stride()) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        wsum_f64(acc, hist, idx, val, n_terms, v, E);
        out[v] = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
    }
}

// fast mode: fp32 history, fp32 FMA accumulate (contraction re-enabled locally)
__global__ __launch_bounds__(kBlock) void k_step_f32hist(
    const float4* __restrict__ x_k, const float4* __restrict__ mout, const float4* __restrict__ noise,
    float* __restrict__ hist, float4* __restrict__ x_next,
    const int32_t* __restrict__ idx, const float* __restrict__ val, int n_terms, float c_diag,
    int k, float inv_alpha, float sigma2_over_std, float b0, int64_t nvec, int64_t E)
{
    for (int64_t v = first_vec(); v < nvec; v += vec_stride()) {
        const float4 xv = x_k[v], ov = mout[v], nv = noise[v];
        float4 x0;
        x0.x = __builtin_fmaf(-ov.x, sigma2_over_std, xv.x) * inv_alpha;
        x0.y = __builtin_fmaf(-ov.y, sigma2_over_std, xv.y) * inv_alpha;
        x0.z = __builtin_fmaf(-ov.z, sigma2_over_std, xv.z) * inv_alpha;
        x0.w = __builtin_fmaf(-ov.w, sigma2_over_std, xv.w) * inv_alpha;
        reinterpret_cast<float4*>(hist + (int64_t)k * E)[v] = x0;
        float4 acc = make_float4(b0 * nv.x, b0 * nv.y, b0 * nv.z, b0 * nv.w);
#pragma unroll 4
        for (int t = 0; t < n_terms; ++t) {
            const float c = val[t];
            const float4 h = reinterpret_cast<const float4*>(hist + (int64_t)idx[t] * E)[v];
            acc.x = __builtin_fmaf(h.x, c, acc.x); acc.y = __builtin_fmaf(h.y, c, acc.y);
            acc.z = __builtin_fmaf(h.z, c, acc.z); acc.w = __builtin_fmaf(h.w, c, acc.w);
        }
        acc.x = __builtin_fmaf(x0.x, c_diag, acc.x); acc.y = __builtin_fmaf(x0.y, c_diag, acc.y);
        acc.z = __builtin_fmaf(x0.z, c_diag, acc.z); acc.w = __builtin_fmaf(x0.w, c_diag, acc.w);
        x_next[v] = acc;
    }
}

__global__ __launch_bounds__(kBlock) void k_to_pixel(
    const float* __restrict__ x, uint8_t* __restrict__ out, int C, int HW, int centered)
{
    // one sample per blockIdx.y; out[(p*C + c)] <- in[c*HW + p]: the C reads of a pixel are HW floats apart
    // (same few cache lines across neighbouring lanes), the byte writes are fully coalesced.
    const float* xs = x + (int64_t)blockIdx.y * C * HW;
    uint8_t* os = out + (int64_t)blockIdx.y * C * HW;
    const int n = C * HW;
    for (int o = blockIdx.x * kBlock + threadIdx.x; o < n; o += gridDim.x * kBlock) {
        const int p = o / C, c = o - p * C;
        float v = xs[c * HW + p];
        if (centered) v = (v + 1.0f) / 2.0f;                 // inverse scaler, datasets.py:32-38
        v = v * 255.0f;
        v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
        os[o] = (uint8_t)(int)v;
    }
}

// ------------------------------------------------------------------------------------------
// Validate form: fp32 products, fp64 accumulate
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_step_f32prod(
    const float4* __restrict__ z, const float* __restrict__ cond, const float* __restrict__ uncond, float cfg,
    int64_t svec, int64_t sstride,
    float* __restrict__ hist_x0, const float* __restrict__ hist_eps, float4* __restrict__ z_next,
    const int32_t* __restrict__ idx_c, const float* __restrict__ val_c, int n_c, float c_diag,
    const int32_t* __restrict__ idx_b, const float* __restrict__ val_b, int n_b,
    int k, float c1, float c2, int64_t nvec, int64_t E)
{
    for (int64_t v = first_vec(); v < nvec; v += vec_stride()) {
        const int64_t img = v / svec, q = v - img * svec;
        const float4 x0 = x0_f32prod(c1, z[v], c2, cfg_eps(cond, uncond, cfg, img, q, sstride));
        double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
        signal_sum_f32prod(a, x0, hist_x0, idx_c, val_c, n_c, c_diag, k, v, E);
        wsum_f32prod(b, hist_eps, idx_b, val_b, n_b, v, E);
        z_next[v] = combine(a, b);
    }
}

__global__ __launch_bounds__(kBlock) void k_wsum_f32prod(
    const float* __restrict__ hist, float4* __restrict__ out,
    const int32_t* __restrict__ idx, const float* __restrict__ val, int n_terms, int64_t nvec, int64_t E)
{
    for (int64_t v = first_vec(); v < nvec; v += vec_stride()) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        wsum_f32prod(a, hist, idx, val, n_terms, v, E);
        out[v] = make_float4((float)a[0], (float)a[1], (float)a[2], (float)a[3]);
    }
}

// ------------------------------------------------------------------------------------------
// SD3 form: all-fp16 chain (every op = fp32 math on fp16 operands, rounded to fp16)
// ------------------------------------------------------------------------------------------
template <bool kVelocityCfg>
__global__ __launch_bounds__(kBlock) void k_step_f16chain(
    const h8* __restrict__ x, const h8* __restrict__ v_text, const h8* __restrict__ v_null,
    const h8* __restrict__ noise, h16* __restrict__ hist, h8* __restrict__ mean_out, h8* __restrict__ x_next,
    const int32_t* __restrict__ idx, const float* __restrict__ val, int n_terms, float c_diag, float w_total,
    int k, float sig, float sig_next, float oms_next, float cfg, int64_t nvec, int64_t E)
{
    for (int64_t v = first_vec(); v < nvec; v += vec_stride()) {
        const h8 f = x0_cfg<kVelocityCfg>(x[v], v_text[v], v_null[v], sig, cfg);
        const h8 mean = chain_mean(f, hist, idx, val, n_terms, c_diag, w_total, k, v, E);
        if (mean_out) mean_out[v] = mean;
        if (x_next) x_next[v] = flow_input(noise[v], mean, sig_next, oms_next);
    }
}

// ------------------------------------------------------------------------------------------
// k_step_f16chain with per-image guidance (x0_cfg_image in place of the launch-wide fuse): the null-prompt velocities are
// compacted to the images that are guided, each image carries its own scale.  Everything behind f is the same composition, so
// with uncond_slot[i] == i and cfg_image[i] == cfg the two kernels give the same bytes.  No Philox state here, so the
// grid-stride loop stays.
// ------------------------------------------------------------------------------------------
template <bool kVelocityCfg>
__global__ __launch_bounds__(kBlock) void k_step_f16chain_guided(
    const h8* __restrict__ x, const h8* __restrict__ v_text, const h8* __restrict__ v_null,
    const float* __restrict__ cfg_image, const int32_t* __restrict__ uncond_slot, int64_t svec,
    const h8* __restrict__ noise, h16* __restrict__ hist, h8* __restrict__ mean_out, h8* __restrict__ x_next,
    const int32_t* __restrict__ idx, const float* __restrict__ val, int n_terms, float c_diag, float w_total,
    int k, float sig, float sig_next, float oms_next, int64_t nvec, int64_t E)
{
    for (int64_t v = first_vec(); v < nvec; v += vec_stride()) {
        const int64_t img = v / svec, q = v - img * svec;            // an image is svec 8-vectors
        const h8 f = x0_cfg_image<kVelocityCfg>(x[v], v_text[v], v_null, cfg_image, uncond_slot, img, q, svec, sig);
        const h8 mean = chain_mean(f, hist, idx, val, n_terms, c_diag, w_total, k, v, E);
        if (mean_out) mean_out[v] = mean;
        if (x_next) x_next[v] = flow_input(noise[v], mean, sig_next, oms_next);
    }
}

__global__ __launch_bounds__(kBlock) void k_flow_input_f16(
    const h8* __restrict__ noise, const h8* __restrict__ mean, h8* __restrict__ out, float sig, float oms, int64_t nvec)
{
    for (int64_t v = first_vec(); v < nvec; v += vec_stride())
        out[v] = flow_input(noise[v], mean ? mean[v] : h8_zero(), sig, oms);
}

__global__ __launch_bounds__(kBlock) void k_wmean_f16(
    const h16* __restrict__ hist, h8* __restrict__ out,
    const int32_t* __restrict__ idx, const float* __restrict__ val, int n_terms, float w_total,
    int64_t nvec, int64_t E)
{
    for (int64_t v = first_vec(); v < nvec; v += vec_stride()) {
        h8 acc = h8_zero();
        chain_terms(acc, hist, idx, val, n_terms, v, E);
        out[v] = mean_of(acc, w_total);
    }
}

// ------------------------------------------------------------------------------------------
// Counter-based initial noise: Philox4x32-10 keyed by (seed, global image index).  The reference draws one
// sequential torch.randn stream (src/CIFAR10NaturalInference.py:285-290), which cannot be sharded; keying
// the generator by the image's GLOBAL index makes image i identical for any GPU count / batch split.
// counter = (index lo, index hi, element quad, 0), key = (seed lo, seed hi); 4 x uint32 -> 4 normals (Box-Muller).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&o)[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// The four normals of one element quad: Philox4x32-10 of counter (gi lo, gi hi, quad lo, word3), then Box-Muller on the
// two pairs.  word3 is quad >> 32 for the initial noise (column 0) and the column j for the noise injected after step
// j-1 (quad < 2^32 then): k_randn_philox and noise_row_sum both call this, so the fused steps inject exactly the normals
// natinf_randn_philox_col_f32 returns.
__device__ __forceinline__ float4 philox_normals(uint64_t gi, uint64_t q, uint32_t word3, uint32_t k0, uint32_t k1)
{
    uint32_t r[4];
    philox4x32_10((uint32_t)gi, (uint32_t)(gi >> 32), (uint32_t)q, word3, k0, k1, r);
    float z[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = ((float)(r[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);       // (0, 1), 24 bits
        const float u2 = ((float)(r[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float rad = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincosf(6.28318530717958647692f * u2, &sn, &cs);
        z[2 * h] = rad * cs; z[2 * h + 1] = rad * sn;
    }
    return make_float4(z[0], z[1], z[2], z[3]);
}

// global index of image img of the batch: from the caller's array, or first + img*stride
__device__ __forceinline__ uint64_t global_index(const int64_t* index, int64_t first, int64_t stride, int64_t img) {
    return (uint64_t)(index ? index[img] : first + img * stride);
}

// acc <- the noise row sum_t val_b[t] * eps_{idx_b[t]} in the Validate form's arithmetic
// (src/ValidateNaturalInference.py:198-204: fp32 product, fp64 accumulate in ascending column order).  eps_0 is the caller's
// noise; eps_j, j >= 1, is generated in registers (philox_normals with word3 = j): what a slab whose row j
// natinf_randn_philox_col_f32(column = j) filled would hold.
__device__ __forceinline__ void noise_row_sum(double (&acc)[4], const float4* noise, const int32_t* idx_b, const float* val_b,
                                              int n_b, int64_t v, uint64_t gi, int64_t q, uint32_t k0, uint32_t k1)
{
    for (int t = 0; t < n_b; ++t) {                               // wave-uniform column: one Philox call per quad and term
        const float c = val_b[t];
        const uint32_t j = (uint32_t)idx_b[t];
        const float4 e = j == 0 ? noise[v] : philox_normals(gi, (uint64_t)q, j, k0, k1);
        acc_prod(acc, e, c);
    }
}

// ---- the step bodies with in-kernel noise, each written here and nowhere else ----
// CIFAR10 form, the tail of element quad v (quad q of its image) once its x0 is final: x0 stored as hist[k], signal sum, diagonal term, noise_row_sum,
// x_next = (float)acc_x0 + (float)acc_eps.  (noise_step_quad; k_stepfix_f64 and k_stepproject_f64 with the corrected / projected quad)
__device__ __forceinline__ float4 noise_step_tail_f64(
    const double (&x0)[4], const float4* noise, double* hist, const int32_t* idx, const double* val, int n_terms, double c_diag,
    const int32_t* idx_b, const float* val_b, int n_b, uint64_t gi, int64_t q, uint32_t k0, uint32_t k1, int k, int64_t v, int64_t E)
{
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, nacc[4] = {0.0, 0.0, 0.0, 0.0};
    st_quad_f64(hist + (int64_t)k * E, v, x0);
    wsum_f64(acc, hist, idx, val, n_terms, v, E);
    acc_f64(acc, x0[0], x0[1], x0[2], x0[3], c_diag);
    noise_row_sum(nacc, noise, idx_b, val_b, n_b, v, gi, q, k0, k1);
    return combine(acc, nacc);
}

// CIFAR10 form, one quad per thread: x0 from the score, then the tail above (k_step_noise_f64, k_step_inpaint_f64, k_step_colorize_f64).  Only the
// unblended float4 leaves: in k_step_colorize_f64 the fp64 accumulators of a plane are dead before the next plane's begin.
__device__ __forceinline__ float4 noise_step_quad(
    const float4* x_k, const float4* mout, const float4* noise, double* hist, const int32_t* idx, const double* val, int n_terms, double c_diag,
    const int32_t* idx_b, const float* val_b, int n_b, uint64_t gi, int64_t q, uint32_t k0, uint32_t k1, int k, double alpha, double sigma2,
    float stdv, int64_t v, int64_t E)
{
    double x0[4];
    x0_score_f64(x0, x_k[v], mout[v], stdv, sigma2, alpha);
    return noise_step_tail_f64(x0, noise, hist, idx, val, n_terms, c_diag, idx_b, val_b, n_b, gi, q, k0, k1, k, v, E);
}

// Validate form, one quad per thread: signal_sum_f32prod, noise_row_sum in place of a hist_eps slab's row sum, combine (the three seeded step kernels)
__device__ __forceinline__ float4 noise_step_f32prod(
    float4 x0, float* hist_x0, const float4* noise, const int32_t* idx_c, const float* val_c, int n_c, float c_diag,
    const int32_t* idx_b, const float* val_b, int n_b, uint64_t gi, int64_t q, uint32_t k0, uint32_t k1, int k, int64_t v, int64_t E)
{
    double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
    signal_sum_f32prod(a, x0, hist_x0, idx_c, val_c, n_c, c_diag, k, v, E);
    noise_row_sum(b, noise, idx_b, val_b, n_b, v, gi, q, k0, k1);
    return combine(a, b);
}

__global__ __launch_bounds__(kBlock) void k_randn_philox(
    float4* __restrict__ out, const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride,
    int64_t quads_per_image, int64_t total_quads, uint32_t column, uint32_t k0, uint32_t k1)
{
    for (int64_t v = first_vec(); v < total_quads; v += vec_stride()) {
        const int64_t img = v / quads_per_image, q = v - img * quads_per_image;
        const uint64_t gi = global_index(index, first_index, index_stride, img);
        out[v] = philox_normals(gi, (uint64_t)q, column ? column : (uint32_t)((uint64_t)q >> 32), k0, k1);
    }
}

// ------------------------------------------------------------------------------------------
// CIFAR10 form with per-step noise (stochastic matrices: B[k, j >= 1] != 0): k_step_f64hist's x0_k and signal sum, then
// noise_row_sum and x_next = (float)acc_x0 + (float)acc_eps.  No noise slab, and every image's noise is a function of
// (seed, global index, column).  A row whose only entry is column 0 gives (float)acc + b0*noise, the bits of k_step_f64hist.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_step_noise_f64(
    const float4* __restrict__ x_k, const float4* __restrict__ mout, const float4* __restrict__ noise,
    double* __restrict__ hist, float4* __restrict__ x_next,
    const int32_t* __restrict__ idx, const double* __restrict__ val, int n_terms, double c_diag,
    const int32_t* __restrict__ idx_b, const float* __restrict__ val_b, int n_b,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride, int64_t quads_per_image,
    uint32_t k0, uint32_t k1, int k, double alpha, double sigma2, float stdv, int64_t nvec, int64_t E)
{
    // one element quad per thread, no grid-stride loop: with the loop's carried scalars the 20 Philox round keys the
    // compiler hoists into SGPRs spill (10-35 SGPRs); without it the kernel needs 57 SGPRs and spills nothing
    const int64_t v = first_vec();
    if (v < nvec) {
        const int64_t img = v / quads_per_image, q = v - img * quads_per_image;
        x_next[v] = noise_step_quad(x_k, mout, noise, hist, idx, val, n_terms, c_diag, idx_b, val_b, n_b,
                                    global_index(index, first_index, index_stride, img), q, k0, k1, k, alpha, sigma2, stdv, v, E);
    }
}

// ---- piece of the inpainting forms: known pixels re-noised to the level of the step's output ----
// quad q of image img, xv the unconditioned value: element i with a non-zero mask byte becomes fp32(fp32(known*alpha) + fp32(z*std)), z the
// Philox normals of column `column` (what natinf_randn_philox_col_f32 returns); the others keep xv.  A SELECT, not x*(1-mask) + md*mask: a NaN
// of the unknown side stays out of the known pixels.  std == 0 (wave-uniform): no draw, fp32(known*alpha).  The draw is also skipped by the
// lanes whose mask word is 0 (a wave without a known pixel branches over it).  The mask is read as one 32-bit word per quad.
__device__ __forceinline__ float4 known_blend(float4 xv, const float* known, const uint8_t* mask, int64_t kstride, int64_t mstride,
                                              int64_t img, int64_t q, int64_t qpi, float alpha, float stdv, uint32_t column,
                                              uint64_t gi, uint32_t k0, uint32_t k1)
{
    // a stride is 0 or 4*qpi: the word index of the quad within the mask, the quad index within known
    const int64_t mq = (mstride ? img * qpi : 0) + q, kq = (kstride ? img * qpi : 0) + q;
    const uint32_t m = reinterpret_cast<const uint32_t*>(mask)[mq];
    const float4 kv = reinterpret_cast<const float4*>(known)[kq];
    float md[4] = {kv.x * alpha, kv.y * alpha, kv.z * alpha, kv.w * alpha};
    if (stdv != 0.0f && m != 0u) {
        const float4 z = philox_normals(gi, (uint64_t)q, column, k0, k1);
        const float n0 = z.x * stdv, n1 = z.y * stdv, n2 = z.z * stdv, n3 = z.w * stdv;
        md[0] = md[0] + n0; md[1] = md[1] + n1; md[2] = md[2] + n2; md[3] = md[3] + n3;
    }
    return make_float4((m & 0x000000FFu) ? md[0] : xv.x, (m & 0x0000FF00u) ? md[1] : xv.y,
                       (m & 0x00FF0000u) ? md[2] : xv.z, (m & 0xFF000000u) ? md[3] : xv.w);
}

// the blend on its own: the first model input of an inpainting trajectory, and the definition the fused step is tested against.
// x_in and out may be the same buffer (a thread reads its quad before it writes it): no __restrict__ on them.
__global__ __launch_bounds__(kBlock) void k_known_blend(
    const float4* x_in, float4* out, const float* __restrict__ known, const uint8_t* __restrict__ mask,
    int64_t kstride, int64_t mstride, float kalpha, float kstd, uint32_t kcolumn,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride, int64_t quads_per_image,
    uint32_t k0, uint32_t k1, int64_t nvec)
{
    // one element quad per thread, no grid-stride loop (k_step_noise_f64)
    const int64_t v = first_vec();
    if (v < nvec) {
        const int64_t img = v / quads_per_image, q = v - img * quads_per_image;
        out[v] = known_blend(x_in[v], known, mask, kstride, mstride, img, q, quads_per_image, kalpha, kstd, kcolumn,
                             global_index(index, first_index, index_stride, img), k0, k1);
    }
}

// ------------------------------------------------------------------------------------------
// CIFAR10 form, inpainting: k_step_noise_f64 operation for operation (hist[k] and the unblended x_next are its bytes), then known_blend in
// registers before the one 16-byte store of x_next: no second pass over x, no noise slab.  x_next equals k_step_noise_f64 followed by
// k_known_blend, byte for byte.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_step_inpaint_f64(
    const float4* __restrict__ x_k, const float4* __restrict__ mout, const float4* __restrict__ noise,
    double* __restrict__ hist, float4* __restrict__ x_next,
    const int32_t* __restrict__ idx, const double* __restrict__ val, int n_terms, double c_diag,
    const int32_t* __restrict__ idx_b, const float* __restrict__ val_b, int n_b,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride, int64_t quads_per_image,
    uint32_t k0, uint32_t k1, int k, double alpha, double sigma2, float stdv,
    const float* __restrict__ known, const uint8_t* __restrict__ mask, int64_t kstride, int64_t mstride,
    float kalpha, float kstd, uint32_t kcolumn, int64_t nvec, int64_t E)
{
    // one element quad per thread, no grid-stride loop (k_step_noise_f64: with one, the hoisted Philox round keys spill SGPRs)
    const int64_t v = first_vec();
    if (v < nvec) {
        const int64_t img = v / quads_per_image, q = v - img * quads_per_image;
        const uint64_t gi = global_index(index, first_index, index_stride, img);
        const float4 xn = noise_step_quad(x_k, mout, noise, hist, idx, val, n_terms, c_diag, idx_b, val_b, n_b, gi, q, k0, k1, k, alpha,
                                          sigma2, stdv, v, E);
        x_next[v] = known_blend(xn, known, mask, kstride, mstride, img, q, quads_per_image, kalpha, kstd, kcolumn, gi, k0, k1);
    }
}

// ---- pieces of the x0 correction (static clip / dynamic thresholding): one workgroup per image, the image's raw x0 in LDS ----
// The LDS of a workgroup: the image as four planes (element i of quad q at x[i][q]: a wave's 8-byte accesses are consecutive, conflict-free)
// and the scratch of the order-statistic search.  kCapQuads is the kernel's capacity; the host picks the instantiation that holds the image.
constexpr int kFixQuadsSmall = 768, kFixQuadsMax = 2048;             // 32x32x3 (24 KB of fp64) and the ABI's cap of 8192 elements (64 KB)
constexpr int kWaves = kBlock / 64;
template <int kCapQuads>
struct FixLds {
    double x[4][kCapQuads];
    unsigned int bins[256];                                         // one radix digit's histogram
    unsigned int wave_total[kWaves];
    unsigned int sel_bin, sel_rank, sel_count, any_nan;
    unsigned long long min_above;
};

// ---- quad <-> planes, for any LDS struct with x[4][...] (FixLds, and ProjLds below) ----
template <class Lds>
__device__ __forceinline__ void st_planes(Lds& L, int q, const double (&x)[4]) { L.x[0][q] = x[0]; L.x[1][q] = x[1]; L.x[2][q] = x[2]; L.x[3][q] = x[3]; }
template <class Lds>
__device__ __forceinline__ void ld_planes(double (&x)[4], const Lds& L, int q) { x[0] = L.x[0][q]; x[1] = L.x[1][q]; x[2] = L.x[2][q]; x[3] = L.x[3][q]; }

// quad q of the planes <- the raw x0 of the image's quad (xv, ov) = (x_k, mout): x0_score_f64, to LDS and nowhere else (k_stepfix_f64, k_stepproject_f64).
// The one-line loop over the thread's quads stays in the kernel: inside a piece the compiler walks x_k / mout with vector pointers, not scalar ones.
template <class Lds>
__device__ __forceinline__ void plane_quad_from_score(Lds& L, int q, float4 xv, float4 ov, float stdv, double sigma2, double alpha) {
    double x0[4];
    x0_score_f64(x0, xv, ov, stdv, sigma2, alpha);
    st_planes(L, q, x0);
}

// the planes <- an image of qpi fp64 quads in memory; back to memory, one quad at a time, is st_quad_f64 (k_x0fix_f64, k_x0project_f64)
template <class Lds>
__device__ __forceinline__ void planes_from_image(Lds& L, const double* img, int qpi) {
    const d2* p = reinterpret_cast<const d2*>(img);
    for (int q = threadIdx.x; q < qpi; q += kBlock) {
        const d2 a = p[2 * q], b = p[2 * q + 1];
        const double x[4] = {a.x, a.y, b.x, b.y};
        st_planes(L, q, x);
    }
}

// |x| as its 64-bit pattern: non-negative doubles order as unsigned integers, NaN patterns sort above +inf
__device__ __forceinline__ uint64_t abs_key(double x) { return (uint64_t)__double_as_longlong(x) & 0x7FFFFFFFFFFFFFFFull; }
constexpr uint64_t kInfKey = 0x7FF0000000000000ull;

// The dynamic threshold of the image in L.x (qpi quads), for every thread of the workgroup: a[lo] and, with `next`, a[lo + 1] of the ascending
// |x| by an 8-bit radix select on the keys (most significant digit first; integer LDS counts, so arrival order cannot matter), then
//   d = a[hi] - a[lo] ; q = w < 0.5 ? fma(w, d, a[lo]) : fma(w - 1, d, a[hi]) ; s = any NaN in x or q NaN ? NaN : max(q, max_val)
// The fma is the file's one fused operation, asked for by name (torch.quantile's interpolation is one).  Every branch around a barrier is
// workgroup-uniform: its condition is read from LDS behind a barrier.
template <int kCapQuads>
__device__ __forceinline__ double dynamic_threshold(FixLds<kCapQuads>& L, int qpi, unsigned lo, bool next, double w, double max_val)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { L.any_nan = 0u; L.min_above = ~0ull; }
    uint64_t prefix = 0;
    unsigned r = lo, count = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        L.bins[tid] = 0u;                                           // kBlock == 256 digits
        __syncthreads();
        const uint64_t himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
        bool nan = false;
        for (int q = tid; q < qpi; q += kBlock) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint64_t key = abs_key(L.x[i][q]);
                nan = nan || key > kInfKey;
                if ((key & himask) == prefix) atomicAdd(&L.bins[(unsigned)(key >> shift) & 0xFFu], 1u);
            }
        }
        if (shift == 56 && nan) atomicOr(&L.any_nan, 1u);
        __syncthreads();
        // the digit whose cumulative count passes r: inclusive scan of the 256 counts (in the wave by lane shifts, across waves through LDS)
        const unsigned c = L.bins[tid];
        unsigned incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) L.wave_total[wave] = incl;
        __syncthreads();
        for (int wv = 0; wv < wave; ++wv) incl += L.wave_total[wv];
        if (incl - c <= r && r < incl) { L.sel_bin = (unsigned)tid; L.sel_rank = r - (incl - c); L.sel_count = c; }      // exactly one thread
        __syncthreads();
        prefix |= (uint64_t)L.sel_bin << shift;
        r = L.sel_rank;
        count = L.sel_count;                                        // after the last digit: how many elements equal a[lo], r its rank among them
    }
    uint64_t hi_key = prefix;
    if (next && r + 1 >= count) {                                   // a[lo] is the last of its value: a[lo + 1] is the least key above it
        uint64_t m = ~0ull;
        for (int q = tid; q < qpi; q += kBlock) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint64_t key = abs_key(L.x[i][q]);
                m = key > prefix && key < m ? key : m;
            }
        }
        if (m != ~0ull) atomicMin(&L.min_above, (unsigned long long)m);
        __syncthreads();
        hi_key = L.min_above;
    }
    const double a_lo = __longlong_as_double((long long)prefix), a_hi = __longlong_as_double((long long)hi_key);
    const double d = a_hi - a_lo;
    const double wm1 = w - 1.0;
    const double q = w < 0.5 ? __builtin_fma(w, d, a_lo) : __builtin_fma(wm1, d, a_hi);
    if (L.any_nan != 0u || q != q) return __builtin_nan("");
    return q > max_val ? q : max_val;
}

// the threshold of the workgroup's image for the mode: max_val itself (CLIP, nothing searched) or dynamic_threshold
template <int kCapQuads>
__device__ __forceinline__ double x0_threshold(FixLds<kCapQuads>& L, int qpi, int mode, unsigned lo, bool next, double w, double max_val) {
    return mode == NATINF_X0_CLIP ? max_val : dynamic_threshold(L, qpi, lo, next, w, max_val);
}

// the corrected quad.  CLIP: x < -c ? -c : (x > c ? c : x), a NaN stays as it is, no division.  DYNAMIC: min(max(x, -s), s) / s, one IEEE fp64
// division; a NaN threshold makes the whole image NaN (both comparisons fail, x / NaN), and every NaN quotient (inf / inf under an infinite
// threshold too) leaves as the one quiet NaN pattern 0x7FF8000000000000.
__device__ __forceinline__ void x0_fix(double (&y)[4], const double (&x)[4], int mode, double s) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double lo = x[i] < -s ? -s : x[i];
        const double t = lo > s ? s : lo;
        const double r = t / s;
        y[i] = mode == NATINF_X0_CLIP ? t : (r != r ? __builtin_nan("") : r);
    }
}

// the correction on its own, in place: the definition the fused step is tested against.  blockIdx.x = image.
template <int kCapQuads>
__global__ __launch_bounds__(kBlock) void k_x0fix_f64(double* x0, double* __restrict__ s_out, int qpi, int mode, unsigned lo, int next,
                                                     double w, double max_val)
{
    __shared__ FixLds<kCapQuads> L;
    const int tid = threadIdx.x;
    double* img = x0 + 4 * (int64_t)blockIdx.x * qpi;
    planes_from_image(L, img, qpi);
    // (a thread reads back only what it wrote itself; the search's first barrier comes before any other thread's read)
    const double s = x0_threshold(L, qpi, mode, lo, next != 0, w, max_val);
    for (int q = tid; q < qpi; q += kBlock) {
        double x[4], y[4];
        ld_planes(x, L, q);
        x0_fix(y, x, mode, s);
        st_quad_f64(img, q, y);
    }
    if (s_out && tid == 0) s_out[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------
// CIFAR10 form with the x0 correction: k_step_inpaint_f64's composition with one workgroup per image (blockIdx.x = image; a thread owns the
// quads tid, tid + kBlock, ...).  The raw x0 of the image goes to LDS and nowhere else; after the threshold is known each quad is corrected,
// stored once as hist[k], and used for the diagonal term; the rest is k_step_noise_f64 operation for operation, then known_blend if there are
// known pixels.  hist[k] equals k_step_noise_f64 followed by k_x0fix_f64, byte for byte.
// ------------------------------------------------------------------------------------------
template <int kCapQuads>
__global__ __launch_bounds__(kBlock) void k_stepfix_f64(
    const float4* __restrict__ x_k, const float4* __restrict__ mout, const float4* __restrict__ noise,
    double* __restrict__ hist, float4* __restrict__ x_next,
    const int32_t* __restrict__ idx, const double* __restrict__ val, int n_terms, double c_diag,
    const int32_t* __restrict__ idx_b, const float* __restrict__ val_b, int n_b,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride, int qpi,
    uint32_t k0, uint32_t k1, int k, double alpha, double sigma2, float stdv,
    const float* __restrict__ known, const uint8_t* __restrict__ mask, int64_t kstride, int64_t mstride,
    float kalpha, float kstd, uint32_t kcolumn,
    int mode, unsigned lo, int next, double w, double max_val, double* __restrict__ s_out, int64_t E)
{
    __shared__ FixLds<kCapQuads> L;
    const int tid = threadIdx.x;
    const int64_t img = blockIdx.x, v0 = img * qpi;
    for (int q = tid; q < qpi; q += kBlock) plane_quad_from_score(L, q, x_k[v0 + q], mout[v0 + q], stdv, sigma2, alpha);
    const double s = x0_threshold(L, qpi, mode, lo, next != 0, w, max_val);
    if (s_out && tid == 0) s_out[img] = s;

    const uint64_t gi = global_index(index, first_index, index_stride, img);
    // the Philox key pinned in vector registers: left scalar, the 20 round keys the compiler derives from it are hoisted out of this loop into
    // SGPRs, next to the loop's own carried scalars, and spill (k_step_noise_f64 drops its loop for that; this kernel's loop is its shape)
    asm("" : "+v"(k0), "+v"(k1));
    for (int q = tid; q < qpi; q += kBlock) {
        const int64_t v = v0 + q;
        double x[4], y[4];
        ld_planes(x, L, q);
        x0_fix(y, x, mode, s);
        float4 xn = noise_step_tail_f64(y, noise, hist, idx, val, n_terms, c_diag, idx_b, val_b, n_b, gi, q, k0, k1, k, v, E);
        if (known) xn = known_blend(xn, known, mask, kstride, mstride, img, q, qpi, kalpha, kstd, kcolumn, gi, k0, k1);
        x_next[v] = xn;
    }
}

// ---- pieces of the x0 projection (super-resolution from a low-resolution picture, DDNM): x0 <- x0 + A+(low - A x0), A the s x s block average of
// an NCHW image, A+ pixel replication.  One workgroup per image, the image's raw x0 in LDS as for the correction above ----
// The LDS of a workgroup: the four planes x[i][q], each padded by kProjPad doubles, and one value per block ROW (the s consecutive elements of one
// image row inside one block; block row br is elements br*s .. br*s + s - 1, since W is a multiple of s): first its sum, then, in the entry of a
// block's top row, the block's residual d.  The pad puts planes two apart (2*(kCapQuads + 8) doubles) half a bank row (128 B) from each other: at
// s = 2 neighbouring lanes read the same quad of planes 0 and 2 (then 1 and 3), which an unpadded plane stride (a multiple of 256 B) would put on
// the same banks.
constexpr int kProjPad = 8;
template <int kCapQuads>
struct ProjLds {
    double x[4][kCapQuads + kProjPad];
    double rs[2 * kCapQuads];                                       // elems / s block rows, s >= 2
    unsigned long long rmax;                                        // max |d| of the image as its 64-bit pattern
};
// the geometry of a call: quads per image, log2 s, blocks per image row (W / s) and the exact fp64 value 2^(-2 log2 s)
struct ProjGeom { int qpi, l2s, wb; double inv; };

// r_j of block row br: its s elements added left to right, started from the first one.  A thread owns a block row: at s = 4 that is quad br
// (consecutive lanes read consecutive 8-byte words of one plane: conflict-free), at s = 8 quads 2br and 2br + 1 (a stride of two words: the 32 lanes
// of a ds_read_b64 group span two bank rows, 2-way), at s = 2 half of quad br / 2 (planes 0, 1 or 2, 3: conflict-free with the pad above).
template <int kCapQuads>
__device__ __forceinline__ double proj_row_sum(const ProjLds<kCapQuads>& L, int br, int l2s) {
    if (l2s == 1) {
        const int q = br >> 1, p = (br & 1) * 2;
        return L.x[p][q] + L.x[p + 1][q];
    }
    int q = br << (l2s - 2);
    double r = L.x[0][q] + L.x[1][q];
    r = r + L.x[2][q];
    r = r + L.x[3][q];
    for (int i = 1; i < (1 << (l2s - 2)); ++i) {
        ++q;
        r = r + L.x[0][q]; r = r + L.x[1][q]; r = r + L.x[2][q]; r = r + L.x[3][q];
    }
    return r;
}

// The residuals of the image in L.x: block row sums (a thread per block row), then a thread per block b = (c, I, J) -- the index of its value in
// `low` -- adds its s row sums top to bottom (rows Wb entries apart), m = S * 2^(-2 log2 s), d = low[b] - m, kept in the entry of the block's top
// row; max |d| by an integer LDS maximum on the 64-bit patterns (a NaN pattern sorts above +inf), so arrival order cannot matter.  Begins with
// the barrier that completes the planes and ends with the one that completes the residuals.
template <int kCapQuads>
__device__ __forceinline__ void x0_project_residuals(ProjLds<kCapQuads>& L, const double* __restrict__ low, ProjGeom g)
{
    const int tid = threadIdx.x;
    const int nbr = (4 * g.qpi) >> g.l2s, nblk = nbr >> g.l2s, s = 1 << g.l2s;
    if (tid == 0) L.rmax = 0ull;
    __syncthreads();
    for (int br = tid; br < nbr; br += kBlock) L.rs[br] = proj_row_sum(L, br, g.l2s);
    __syncthreads();
    uint64_t mx = 0;
    for (int b = tid; b < nblk; b += kBlock) {
        const unsigned grp = (unsigned)b / (unsigned)g.wb, J = (unsigned)b - grp * (unsigned)g.wb;       // grp = c * (H / s) + I
        const int br0 = (int)((grp << g.l2s) * (unsigned)g.wb + J);
        double S = L.rs[br0];
        for (int j = 1; j < s; ++j) S = S + L.rs[br0 + j * g.wb];
        const double m = S * g.inv;
        const double d = low[b] - m;
        L.rs[br0] = d;                                              // (no other thread reads or writes this block's entries)
        const uint64_t key = abs_key(d);
        mx = key > mx ? key : mx;
    }
    if (mx) atomicMax(&L.rmax, (unsigned long long)mx);
    __syncthreads();
}

// r of the workgroup's image: max |d|, a NaN maximum as the one quiet NaN
template <int kCapQuads>
__device__ __forceinline__ double proj_r(const ProjLds<kCapQuads>& L) {
    const uint64_t key = L.rmax;
    return key > kInfKey ? __builtin_nan("") : __longlong_as_double((long long)key);
}

// the residual of the block that holds elements e and e + 1, e even (a block row starts at a multiple of s >= 2): row rr = c * H + r of block row
// e / s, its block's top row rr - rr % s (H is a multiple of s)
template <int kCapQuads>
__device__ __forceinline__ double proj_d(const ProjLds<kCapQuads>& L, int e, ProjGeom g) {
    const unsigned br = (unsigned)e >> g.l2s, rr = br / (unsigned)g.wb, J = br - rr * (unsigned)g.wb;
    return L.rs[(rr & ~((1u << g.l2s) - 1u)) * (unsigned)g.wb + J];
}

// the projected quad q: y = x + d, one fp64 addition; a NaN result leaves as the one quiet NaN pattern.  A quad may straddle two block rows (s = 2)
// and, when W is no multiple of 4, two image rows or planes: its two halves are looked up separately.
template <int kCapQuads>
__device__ __forceinline__ void x0_project(double (&y)[4], const ProjLds<kCapQuads>& L, int q, ProjGeom g) {
    double x[4];
    ld_planes(x, L, q);
    const double d[2] = {proj_d(L, 4 * q, g), proj_d(L, 4 * q + 2, g)};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double r = x[i] + d[i >> 1];
        y[i] = r != r ? __builtin_nan("") : r;
    }
}

// the projection on its own, in place: the definition the fused step is tested against.  blockIdx.x = image; lstride = 0 or blocks per image.
template <int kCapQuads>
__global__ __launch_bounds__(kBlock) void k_x0project_f64(double* x0, const double* __restrict__ low, double* __restrict__ r_out, int64_t lstride,
                                                         ProjGeom g)
{
    __shared__ ProjLds<kCapQuads> L;
    const int tid = threadIdx.x;
    double* img = x0 + 4 * (int64_t)blockIdx.x * g.qpi;
    planes_from_image(L, img, g.qpi);
    x0_project_residuals(L, low + (int64_t)blockIdx.x * lstride, g);
    for (int q = tid; q < g.qpi; q += kBlock) {
        double y[4];
        x0_project(y, L, q, g);
        st_quad_f64(img, q, y);
    }
    if (r_out && tid == 0) r_out[blockIdx.x] = proj_r(L);
}

// ------------------------------------------------------------------------------------------
// CIFAR10 form with the x0 projection: k_stepfix_f64's shape (blockIdx.x = image; a thread owns the quads tid, tid + kBlock, ...).  The raw x0 of
// the image goes to LDS and nowhere else; after the residuals are known each quad is projected, stored once as hist[k], and used for the diagonal
// term; the rest is k_step_noise_f64 operation for operation.  hist[k] equals k_step_noise_f64 followed by k_x0project_f64, byte for byte.
// ------------------------------------------------------------------------------------------
template <int kCapQuads>
__global__ __launch_bounds__(kBlock) void k_stepproject_f64(
    const float4* __restrict__ x_k, const float4* __restrict__ mout, const float4* __restrict__ noise,
    double* __restrict__ hist, float4* __restrict__ x_next,
    const int32_t* __restrict__ idx, const double* __restrict__ val, int n_terms, double c_diag,
    const int32_t* __restrict__ idx_b, const float* __restrict__ val_b, int n_b,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride,
    uint32_t k0, uint32_t k1, int k, double alpha, double sigma2, float stdv,
    const double* __restrict__ low, int64_t lstride, ProjGeom g, double* __restrict__ r_out, int64_t E)
{
    __shared__ ProjLds<kCapQuads> L;
    const int tid = threadIdx.x;
    const int64_t img = blockIdx.x, v0 = img * g.qpi;
    for (int q = tid; q < g.qpi; q += kBlock) plane_quad_from_score(L, q, x_k[v0 + q], mout[v0 + q], stdv, sigma2, alpha);
    x0_project_residuals(L, low + img * lstride, g);
    if (r_out && tid == 0) r_out[img] = proj_r(L);

    const uint64_t gi = global_index(index, first_index, index_stride, img);
    // the Philox key pinned in vector registers, as in k_stepfix_f64 and for its reason: left scalar, the 20 round keys hoisted out of this loop spill
    asm("" : "+v"(k0), "+v"(k1));
    for (int q = tid; q < g.qpi; q += kBlock) {
        const int64_t v = v0 + q;
        double y[4];
        x0_project(y, L, q, g);
        x_next[v] = noise_step_tail_f64(y, noise, hist, idx, val, n_terms, c_diag, idx_b, val_b, n_b, gi, q, k0, k1, k, v, E);
    }
}

// ---- pieces of the colorization forms: the gray channel of a rotated colour space re-noised to the level of the step's output ----
// a 3x3 fp32 matrix carried to the kernel by value, row-major m[3*i + j] = M[i][j]: the caller's basis or its inverse, neither is hard-coded here
struct mat3 { float m[9]; };

// fp32( fp32( fp32(a*p) + fp32(b*q) ) + fp32(c*r) ): three products, two sums, five roundings in this order (deps/score_sde_pytorch/
// controllable_generation.py:115,119 is an einsum over the channel index; this is its ascending-index evaluation)
__device__ __forceinline__ float dot3(float a, float b, float c, float p, float q, float r) {
    const float ap = a * p, bq = b * q, cr = c * r;
    const float s = ap + bq;
    return s + cr;
}

// pixel quad pq of image img, x[c] the unconditioned values of plane c (one pixel per lane): rotate (x0, x1, x2) with M, replace latent channel 0
// by fp32(fp32(gray_u*alpha) + fp32(z*std)), z the Philox normals of column `column` for plane 0 (the element quad of plane 0 IS the pixel quad:
// what natinf_randn_philox_col_f32 returns there), rotate back with W.  The old channel 0 is fully replaced, so it is never computed.
// std == 0 (wave-uniform): no draw, fp32(gray_u*alpha).  Unlike known_blend's select, a NaN of x reaches all three outputs of its pixel: that is
// the rotation.  A stride is 0 or the pixel count of an image: gq is the quad index within gray_u.
__device__ __forceinline__ void color_blend(float4 (&x)[3], const float* gray_u, int64_t gq, const mat3& M, const mat3& W,
                                            float alpha, float stdv, uint32_t column, uint64_t gi, int64_t pq, uint32_t k0, uint32_t k1)
{
    const float4 gv = reinterpret_cast<const float4*>(gray_u)[gq];
    float u0[4] = {gv.x * alpha, gv.y * alpha, gv.z * alpha, gv.w * alpha};
    if (stdv != 0.0f) {
        const float4 z = philox_normals(gi, (uint64_t)pq, column, k0, k1);
        const float n0 = z.x * stdv, n1 = z.y * stdv, n2 = z.z * stdv, n3 = z.w * stdv;
        u0[0] = u0[0] + n0; u0[1] = u0[1] + n1; u0[2] = u0[2] + n2; u0[3] = u0[3] + n3;
    }
    const float a[4] = {x[0].x, x[0].y, x[0].z, x[0].w}, b[4] = {x[1].x, x[1].y, x[1].z, x[1].w}, c[4] = {x[2].x, x[2].y, x[2].z, x[2].w};
    float o[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float u1 = dot3(a[i], b[i], c[i], M.m[1], M.m[4], M.m[7]);
        const float u2 = dot3(a[i], b[i], c[i], M.m[2], M.m[5], M.m[8]);
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j][i] = dot3(u0[i], u1, u2, W.m[j], W.m[3 + j], W.m[6 + j]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        // the empty asm pins the four results of a plane in VGPRs at one point: without it the backend, which pairs the lanes into packed fp32
        // operations, stores a quad as two 8-byte halves as each pair becomes ready
        asm("" : "+v"(o[j][0]), "+v"(o[j][1]), "+v"(o[j][2]), "+v"(o[j][3]));
        x[j] = make_float4(o[j][0], o[j][1], o[j][2], o[j][3]);
    }
}

// the blend on its own: the first model input of a colorization trajectory, and the definition the fused step is tested against.  One pixel quad
// per thread: its three element quads sit ppq quads apart (NCHW).  x_in and out may be the same buffer (a thread reads its three quads before it
// writes them, and no other thread touches them): no __restrict__ on them.
__global__ __launch_bounds__(kBlock) void k_color_blend(
    const float4* x_in, float4* out, const float* __restrict__ gray_u, int64_t gstride, mat3 M, mat3 W,
    float galpha, float gstd, uint32_t gcolumn,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride, int64_t ppq,
    uint32_t k0, uint32_t k1, int64_t npq)
{
    // no grid-stride loop (k_step_noise_f64)
    const int64_t t = first_vec();
    if (t < npq) {
        const int64_t img = t / ppq, pq = t - img * ppq, v0 = img * 3 * ppq + pq;
        float4 x[3] = {x_in[v0], x_in[v0 + ppq], x_in[v0 + 2 * ppq]};
        color_blend(x, gray_u, (gstride ? img * ppq : 0) + pq, M, W, galpha, gstd, gcolumn,
                    global_index(index, first_index, index_stride, img), pq, k0, k1);
        out[v0] = x[0]; out[v0 + ppq] = x[1]; out[v0 + 2 * ppq] = x[2];
    }
}

// ------------------------------------------------------------------------------------------
// CIFAR10 form, colorization: one thread per PIXEL quad.  For each plane the thread runs k_step_noise_f64's body on that plane's element quad
// (hist[k] and the unblended values are that kernel's bytes) and keeps the resulting float4 only, then color_blend on the three in registers and
// three 16-byte stores: x_next equals k_step_noise_f64 followed by k_color_blend, byte for byte.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_step_colorize_f64(
    const float4* __restrict__ x_k, const float4* __restrict__ mout, const float4* __restrict__ noise,
    double* __restrict__ hist, float4* __restrict__ x_next,
    const int32_t* __restrict__ idx, const double* __restrict__ val, int n_terms, double c_diag,
    const int32_t* __restrict__ idx_b, const float* __restrict__ val_b, int n_b,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride, int64_t ppq,
    uint32_t k0, uint32_t k1, int k, double alpha, double sigma2, float stdv,
    const float* __restrict__ gray_u, int64_t gstride, mat3 M, mat3 W, float galpha, float gstd, uint32_t gcolumn,
    int64_t npq, int64_t E)
{
    // one pixel quad per thread, no grid-stride loop (k_step_noise_f64: with one, the hoisted Philox round keys spill SGPRs)
    const int64_t t = first_vec();
    if (t < npq) {
        const int64_t img = t / ppq, pq = t - img * ppq, v0 = img * 3 * ppq + pq;
        const uint64_t gi = global_index(index, first_index, index_stride, img);
        float4 x[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            x[c] = noise_step_quad(x_k, mout, noise, hist, idx, val, n_terms, c_diag, idx_b, val_b, n_b, gi, c * ppq + pq, k0, k1, k, alpha,
                                   sigma2, stdv, v0 + c * ppq, E);
        color_blend(x, gray_u, (gstride ? img * ppq : 0) + pq, M, W, galpha, gstd, gcolumn, gi, pq, k0, k1);
        x_next[v0] = x[0]; x_next[v0 + ppq] = x[1]; x_next[v0 + 2 * ppq] = x[2];
    }
}

// ------------------------------------------------------------------------------------------
// Validate form with the noise row generated in registers: k_step_f32prod with noise_row_sum in place of the row sum over a
// hist_eps slab, so the two kernels give the same bytes and the (N+1) x E slab is gone.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_step_noise_f32prod(
    const float4* __restrict__ z, const float* __restrict__ cond, const float* __restrict__ uncond, float cfg,
    int64_t svec, int64_t sstride,
    float* __restrict__ hist_x0, const float4* __restrict__ noise, float4* __restrict__ z_next,
    const int32_t* __restrict__ idx_c, const float* __restrict__ val_c, int n_c, float c_diag,
    const int32_t* __restrict__ idx_b, const float* __restrict__ val_b, int n_b,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride,
    uint32_t k0, uint32_t k1, int k, float c1, float c2, int64_t nvec, int64_t E)
{
    // one element quad per thread, no grid-stride loop (k_step_noise_f64: with one, the hoisted Philox round keys spill SGPRs)
    const int64_t v = first_vec();
    if (v < nvec) {
        const int64_t img = v / svec, q = v - img * svec;            // an image is one sample: svec quads
        const float4 x0 = x0_f32prod(c1, z[v], c2, cfg_eps(cond, uncond, cfg, img, q, sstride));
        z_next[v] = noise_step_f32prod(x0, hist_x0, noise, idx_c, val_c, n_c, c_diag, idx_b, val_b, n_b,
                                       global_index(index, first_index, index_stride, img), q, k0, k1, k, v, E);
    }
}

// ------------------------------------------------------------------------------------------
// k_step_noise_f32prod with per-image guidance (cfg_eps_image in place of cfg_eps): the unconditional rows are compacted to
// the images that are guided, each image carries its own scale.  Everything behind eps is the same composition, so with
// uncond_slot[i] == i and cfg_image[i] == cfg the two kernels give the same bytes.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_step_guided_f32prod(
    const float4* __restrict__ z, const float* __restrict__ cond, const float* __restrict__ uncond,
    const float* __restrict__ cfg_image, const int32_t* __restrict__ uncond_slot, int64_t svec, int64_t sstride,
    float* __restrict__ hist_x0, const float4* __restrict__ noise, float4* __restrict__ z_next,
    const int32_t* __restrict__ idx_c, const float* __restrict__ val_c, int n_c, float c_diag,
    const int32_t* __restrict__ idx_b, const float* __restrict__ val_b, int n_b,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride,
    uint32_t k0, uint32_t k1, int k, float c1, float c2, int64_t nvec, int64_t E)
{
    // one element quad per thread, no grid-stride loop (k_step_noise_f64: with one, the hoisted Philox round keys spill SGPRs)
    const int64_t v = first_vec();
    if (v < nvec) {
        const int64_t img = v / svec, q = v - img * svec;            // an image is one sample: svec quads
        const float4 x0 = x0_f32prod(c1, z[v], c2, cfg_eps_image(cond, uncond, cfg_image, uncond_slot, img, q, sstride));
        z_next[v] = noise_step_f32prod(x0, hist_x0, noise, idx_c, val_c, n_c, c_diag, idx_b, val_b, n_b,
                                       global_index(index, first_index, index_stride, img), q, k0, k1, k, v, E);
    }
}

// ------------------------------------------------------------------------------------------
// Validate form, inpainting: k_step_guided_f32prod operation for operation (hist_x0[k] and the unblended z_next are its bytes), then known_blend
// in registers before the one 16-byte store of z_next: no second pass over z, no noise slab.  The blend's quads-per-image is the sample's svec, and
// it shares the step's global index and Philox key.  z_next equals k_step_guided_f32prod followed by k_known_blend, byte for byte.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_step_inpaint_f32prod(
    const float4* __restrict__ z, const float* __restrict__ cond, const float* __restrict__ uncond,
    const float* __restrict__ cfg_image, const int32_t* __restrict__ uncond_slot, int64_t svec, int64_t sstride,
    float* __restrict__ hist_x0, const float4* __restrict__ noise, float4* __restrict__ z_next,
    const int32_t* __restrict__ idx_c, const float* __restrict__ val_c, int n_c, float c_diag,
    const int32_t* __restrict__ idx_b, const float* __restrict__ val_b, int n_b,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride,
    uint32_t k0, uint32_t k1, int k, float c1, float c2,
    const float* __restrict__ known, const uint8_t* __restrict__ mask, int64_t kstride, int64_t mstride,
    float kalpha, float kstd, uint32_t kcolumn, int64_t nvec, int64_t E)
{
    // one element quad per thread, no grid-stride loop (k_step_noise_f64: with one, the hoisted Philox round keys spill SGPRs)
    const int64_t v = first_vec();
    if (v < nvec) {
        const int64_t img = v / svec, q = v - img * svec;            // an image is one sample: svec quads
        const float4 x0 = x0_f32prod(c1, z[v], c2, cfg_eps_image(cond, uncond, cfg_image, uncond_slot, img, q, sstride));
        const uint64_t gi = global_index(index, first_index, index_stride, img);
        const float4 zn = noise_step_f32prod(x0, hist_x0, noise, idx_c, val_c, n_c, c_diag, idx_b, val_b, n_b, gi, q, k0, k1, k, v, E);
        z_next[v] = known_blend(zn, known, mask, kstride, mstride, img, q, svec, kalpha, kstd, kcolumn, gi, k0, k1);
    }
}

// ---- pieces of the SD3 inpainting form: known latents re-noised to the flow level of the step's output (fp16 chain) ----
// the noise side of 8-vector q of an image in "fresh" mode: the Philox normals of quads 2q and 2q + 1 of column `column` (what
// natinf_randn_philox_col_f32 returns for those eight elements), each rounded to fp16 once
__device__ __forceinline__ h8 philox_h8(uint64_t gi, int64_t q, uint32_t column, uint32_t k0, uint32_t k1) {
    const float4 a = philox_normals(gi, (uint64_t)(2 * q), column, k0, k1), b = philox_normals(gi, (uint64_t)(2 * q + 1), column, k0, k1);
    h8 r;
    r.v[0] = (h16)a.x; r.v[1] = (h16)a.y; r.v[2] = (h16)a.z; r.v[3] = (h16)a.w;
    r.v[4] = (h16)b.x; r.v[5] = (h16)b.y; r.v[6] = (h16)b.z; r.v[7] = (h16)b.w;
    return r;
}

// element i of the result is kn where byte i of the mask word m is non-zero, xv elsewhere.  A SELECT, as in known_blend: a NaN of xv stays out of
// the known elements.
__device__ __forceinline__ h8 select_known(uint64_t m, h8 kn, h8 xv) {
    h8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = ((m >> (8 * i)) & 0xFFull) ? kn.v[i] : xv.v[i];
    return r;
}

// 8-vector i of p as ONE 16-byte load: the empty asm pins the four dwords in VGPRs at one point; without it the backend, which pairs the halves
// the way the selects behind it use them, splits the load of the step's noise vector into 2- and 4-byte pieces
__device__ __forceinline__ h8 ld_whole(const h8* p, int64_t i) {
    float4 raw = reinterpret_cast<const float4*>(p)[i];
    asm("" : "+v"(raw.x), "+v"(raw.y), "+v"(raw.z), "+v"(raw.w));
    h8 r;
    __builtin_memcpy(&r, &raw, sizeof(r));
    return r;
}

// 8-vector q of an image, xv the unconditioned value, m the 8-vector's mask word (not 0) and kv its known values: an element with a non-zero
// mask byte becomes flow_input(n, known, sig, oms) = fp16(fp16(sig*n) + fp16(oms*known)), the rounding order of natinf_flow_input_f16 with
// mean = known.  n is `same` (the image's own initial noise, column == 0) or philox_h8 of the column.  The callers branch over this, and over
// the load of kv, where the mask word is 0: such a thread draws nothing and does not read `known`.
__device__ __forceinline__ h8 known_blend_h8(h8 xv, uint64_t m, h8 same, h8 kv, float sig, float oms, uint32_t column,
                                             uint64_t gi, int64_t q, uint32_t k0, uint32_t k1)
{
    const h8 nz = column ? philox_h8(gi, q, column, k0, k1) : same;
    return select_known(m, flow_input(nz, kv, sig, oms), xv);
}

// the blend on its own: the first model input of an SD3 inpainting trajectory, and the definition the fused step is tested against.
// x_in and out may be the same buffer (a thread reads its 8-vector before it writes it): no __restrict__ on them.
__global__ __launch_bounds__(kBlock) void k_blend_known_f16(
    const h8* x_in, h8* out, const h8* __restrict__ noise, const h8* __restrict__ known, const uint8_t* __restrict__ mask,
    int64_t kstride, int64_t mstride, float sig, float oms, uint32_t column,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride, int64_t svec,
    uint32_t k0, uint32_t k1, int64_t nvec)
{
    // one 8-vector per thread, no grid-stride loop (k_step_noise_f64)
    const int64_t v = first_vec();
    if (v < nvec) {
        const int64_t img = v / svec, q = v - img * svec;
        // a stride is 0 or 8*svec: the word index of the 8-vector within the mask, the vector index within known
        const uint64_t m = reinterpret_cast<const uint64_t*>(mask)[(mstride ? img * svec : 0) + q];
        h8 xv = x_in[v];
        if (m != 0ull)
            xv = known_blend_h8(xv, m, column ? h8_zero() : noise[v], ld_whole(known, (kstride ? img * svec : 0) + q), sig, oms, column,
                                global_index(index, first_index, index_stride, img), q, k0, k1);
        out[v] = xv;
    }
}

// ------------------------------------------------------------------------------------------
// SD3 form, inpainting: k_step_f16chain_guided operation for operation (hist[k], the mean and the unblended x_next are its bytes), then
// known_blend_h8 at the step's own next level (sig_next, oms_next) in registers before the one 16-byte store of x_next: no second pass over x.
// x_next equals k_step_f16chain_guided followed by k_blend_known_f16, byte for byte; "same" mode reuses the noise vector the flow input loaded.
// blend_mean (wave-uniform; the job's last step): mean_out gets `known` itself at the known elements -- the job returns the mean, not x_next.
// ------------------------------------------------------------------------------------------
template <bool kVelocityCfg>
__global__ __launch_bounds__(kBlock) void k_step_inpaint_f16chain(
    const h8* __restrict__ x, const h8* __restrict__ v_text, const h8* __restrict__ v_null,
    const float* __restrict__ cfg_image, const int32_t* __restrict__ uncond_slot, int64_t svec,
    const h8* __restrict__ noise, h16* __restrict__ hist, h8* __restrict__ mean_out, h8* __restrict__ x_next,
    const int32_t* __restrict__ idx, const float* __restrict__ val, int n_terms, float c_diag, float w_total,
    int k, float sig, float sig_next, float oms_next,
    const h8* __restrict__ known, const uint8_t* __restrict__ mask, int64_t kstride, int64_t mstride, uint32_t column, int blend_mean,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride, uint32_t k0, uint32_t k1,
    int64_t nvec, int64_t E)
{
    // one 8-vector per thread, no grid-stride loop (k_step_noise_f64: with one, the hoisted Philox round keys spill SGPRs)
    const int64_t v = first_vec();
    if (v < nvec) {
        const int64_t img = v / svec, q = v - img * svec;            // an image is svec 8-vectors
        const h8 f = x0_cfg_image<kVelocityCfg>(x[v], v_text[v], v_null, cfg_image, uncond_slot, img, q, svec, sig);
        h8 mean = chain_mean(f, hist, idx, val, n_terms, c_diag, w_total, k, v, E);

        const uint64_t m = reinterpret_cast<const uint64_t*>(mask)[(mstride ? img * svec : 0) + q];
        h8 kv = h8_zero(), xn = h8_zero();
        if (m != 0ull) kv = ld_whole(known, (kstride ? img * svec : 0) + q);
        if (x_next) {
            const h8 nv = ld_whole(noise, v);
            xn = flow_input(nv, mean, sig_next, oms_next);
            if (m != 0ull)
                xn = known_blend_h8(xn, m, nv, kv, sig_next, oms_next, column, global_index(index, first_index, index_stride, img), q, k0, k1);
        }
        if (blend_mean) mean = select_known(m, kv, mean);
        if (mean_out) mean_out[v] = mean;
        if (x_next) x_next[v] = xn;
    }
}

// ------------------------------------------------------------------------------------------
// AutoencoderKL posterior (include/natinf_vae.h, natinf_vae_posterior_f32; the last launch of natinf_vae_encode): one thread per element quad
// of the latents.  An image's moments are [mean: C*hw][logvar: C*hw], so quad q of the latents reads quad q of each half: two 16-byte loads, one
// 16-byte store.  std*eps, mean + that, z - shift and its product with scale are four fp32 roundings; eps = philox_normals of the posterior
// column, what natinf_randn_philox_col_f32 returns for (seed, global index, element).  sample == 0 (wave-uniform): no draw, the logvar half is not read.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_vae_posterior(
    const float4* __restrict__ moments, float4* __restrict__ latents, int sample, float scale, float shift,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride, int64_t quads_per_image,
    uint32_t k0, uint32_t k1, int64_t nvec)
{
    // one element quad per thread, no grid-stride loop (k_step_noise_f64)
    const int64_t v = first_vec();
    if (v < nvec) {
        const int64_t img = v / quads_per_image, q = v - img * quads_per_image;
        const float4 mu = moments[2 * img * quads_per_image + q];
        float z[4] = {mu.x, mu.y, mu.z, mu.w};
        if (sample) {
            const float4 lv = moments[(2 * img + 1) * quads_per_image + q];
            const float4 e = philox_normals(global_index(index, first_index, index_stride, img), (uint64_t)q, NATINF_VAE_POSTERIOR_COLUMN, k0, k1);
            const float s0 = expf(0.5f * fminf(fmaxf(lv.x, -30.0f), 20.0f)), s1 = expf(0.5f * fminf(fmaxf(lv.y, -30.0f), 20.0f));
            const float s2 = expf(0.5f * fminf(fmaxf(lv.z, -30.0f), 20.0f)), s3 = expf(0.5f * fminf(fmaxf(lv.w, -30.0f), 20.0f));
            const float n0 = s0 * e.x, n1 = s1 * e.y, n2 = s2 * e.z, n3 = s3 * e.w;
            z[0] = z[0] + n0; z[1] = z[1] + n1; z[2] = z[2] + n2; z[3] = z[3] + n3;
        }
        const float d0 = z[0] - shift, d1 = z[1] - shift, d2 = z[2] - shift, d3 = z[3] - shift;
        latents[v] = make_float4(d0 * scale, d1 * scale, d2 * scale, d3 * scale);
    }
}

// ------------------------------------------------------------------------------------------
// Posterior statistics (include/natinf_posterior.h, natinf_posterior_samples): block (x, row) takes 8 elements of row `row` per thread.  One 16-byte load
// of f (bf16), eps from two 16-byte loads of the caller's slab or two philox_normals quads of column 0 (what natinf_randn_philox_f32 returns for the
// row's global index, elems_per_image = d), s = fl(fl(f*a) + fl(eps*b)), then the exact split s = hi + mid + lo into bf16 (round to nearest even; each
// residual is exact in fp32): three 16-byte stores, one per plane.  The row is uniform over the block, so its global index is a scalar load.
// ------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(kBlock) void k_post_samples(
    const bf16x8* __restrict__ f, const float4* __restrict__ noise, float a, float b,
    const int64_t* __restrict__ index, int64_t first_index, int64_t index_stride, uint32_t k0, uint32_t k1,
    int d8, int64_t plane_vecs, bf16x8* __restrict__ planes)
{
    const int c = blockIdx.x * kBlock + threadIdx.x, row = blockIdx.y;
    if (c < d8) {
        const int64_t v = (int64_t)row * d8 + c;
        const bf16x8 fv = f[v];
        float4 e0, e1;
        if (noise) {
            e0 = noise[2 * v]; e1 = noise[2 * v + 1];
        } else {
            const uint64_t gi = global_index(index, first_index, index_stride, row);
            e0 = philox_normals(gi, (uint64_t)(2 * c), 0u, k0, k1);
            e1 = philox_normals(gi, (uint64_t)(2 * c + 1), 0u, k0, k1);
        }
        const float eps[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
        bf16x8 hi, mid, lo;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float fa = (float)fv[i] * a, eb = eps[i] * b;
            const float s = fa + eb;
            hi[i] = (__bf16)s;
            const float r1 = s - (float)hi[i];
            mid[i] = (__bf16)r1;
            const float r2 = r1 - (float)mid[i];
            lo[i] = (__bf16)r2;
        }
        planes[v] = hi;
        planes[plane_vecs + v] = mid;
        planes[2 * plane_vecs + v] = lo;
    }
}

// ---- host side: argument checks and launch geometry shared by the ABI entries ----
inline int launched() { return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH; }
inline bool terms_ok(const void* idx, const void* val, int n) { return n >= 0 && (n == 0 || (idx && val)); }

// E / lanes vectors when E is a positive multiple of lanes (4 or 8); 0 = refuse
inline int64_t vec_count(int64_t E, int lanes) { return E > 0 && !(E & (lanes - 1)) ? E / lanes : 0; }

// a per-image (per-sample) element count: a positive multiple of lanes (4 or 8) dividing E
inline bool image_ok(int64_t elems, int64_t E, int lanes = 4) { return elems > 0 && !(elems & (lanes - 1)) && !(E % elems); }

// blocks of a one-quad-per-thread launch (k_step_noise_f64, k_step_noise_f32prod); 0 = more than a grid holds
inline unsigned quad_blocks(int64_t nvec) {
    const int64_t blocks = (nvec + kBlock - 1) / kBlock;
    return blocks > INT32_MAX ? 0u : (unsigned)blocks;
}

inline uint32_t seed_lo(uint64_t seed) { return (uint32_t)seed; }              // the two halves of a seed: the Philox key (k0, k1)
inline uint32_t seed_hi(uint64_t seed) { return (uint32_t)(seed >> 32); }

// what every noise-drawing f64 entry (natinf_step_f64hist_noise, _inpaint, _x0fix, _project, _colorize) refuses: a missing tensor, a bad signal or noise
// row, k < 0, E no positive multiple of 4 (nvec == 0), an elems_per_image that is no image of E.  How large an image or a grid may be is each entry's own.
inline bool step_f64_noise_ok(const float* x_k, const float* model_out, const float* noise, const double* hist, const float* x_next, const int32_t* idx,
                              const double* val, int n_terms, const int32_t* idx_b, const float* val_b, int n_b, int k, int64_t nvec, int64_t epi, int64_t E)
{
    return x_k && model_out && noise && hist && x_next && terms_ok(idx, val, n_terms) && terms_ok(idx_b, val_b, n_b) && k >= 0 && nvec && image_ok(epi, E);
}

// what every seeded f32prod entry (natinf_step_f32prod_noise, _noise_guided, _inpaint) refuses before its read-backs: a missing tensor, a bad row, k < 0,
// a noise row longer than its k + 2 columns, a bad E, sample or eps stride, a sample whose quads do not fit counter word 2, a grid too large (blocks == 0)
inline bool step_f32prod_seeded_ok(const float* z, const float* cond, const float* hist_x0, const float* z_next, const int32_t* idx_c, const float* val_c,
                                   int n_c, const int32_t* idx_b, const float* val_b, int n_b, int k, int64_t nvec, unsigned blocks, int64_t sample_elems,
                                   int64_t eps_sample_stride, int64_t E) {
    return z && cond && hist_x0 && z_next && terms_ok(idx_c, val_c, n_c) && terms_ok(idx_b, val_b, n_b) && k >= 0 && n_b <= (int64_t)k + 2 &&
           nvec && image_ok(sample_elems, E) && eps_sample_stride >= sample_elems && !(eps_sample_stride & 3) &&
           !((sample_elems / 4) >> 32) && blocks;
}

// per-image guidance: scales and slots given, and unconditional rows to read when there are any
inline bool guidance_ok(const float* cfg_image, const int32_t* uncond_slot, int n_uncond, const void* uncond) {
    return cfg_image && uncond_slot && n_uncond >= 0 && (n_uncond == 0 || uncond);
}

// the known pixels of an inpainting call: both arrays given, each per-image stride 0 (one row shared by every image) or elems_per_image,
// the mask readable as 32-bit words, and a replacement column no noise column of a matrix (<= N + 1) can collide with
inline bool known_ok(const float* known, const uint8_t* mask, int64_t kstride, int64_t mstride, uint32_t column, int64_t elems_per_image) {
    return known && mask && (kstride == 0 || kstride == elems_per_image) && (mstride == 0 || mstride == elems_per_image) &&
           !((uintptr_t)mask & 3) && column >= 0x80000000u;
}

// the known latents of an SD3 inpainting call: both arrays given, each per-image stride 0 or elems_per_image, the mask readable as 64-bit words,
// an image's quads within counter word 2, and the column 0 ("same": the image's own initial noise, which must be there to read) or a
// replacement column >= 2^31 ("fresh")
inline bool known_ok_f16(const void* known, const uint8_t* mask, int64_t kstride, int64_t mstride, uint32_t column, int64_t elems_per_image,
                         bool have_noise) {
    return known && mask && (kstride == 0 || kstride == elems_per_image) && (mstride == 0 || mstride == elems_per_image) &&
           !((uintptr_t)mask & 7) && !((elems_per_image / 4) >> 32) && (column == 0 ? have_noise : column >= 0x80000000u);
}

// the gray channel of a colorization call: the array and both matrices given, the image three planes of whole quads, a per-image stride of 0 (one
// picture shared by every image) or the pixel count, and a column of the colorization family (>= 2^31 + 2^30: above the inpainting draws' levels)
inline bool gray_ok(const float* gray_u, const float* basis, const float* inverse, int64_t gstride, uint32_t column, int64_t elems_per_image) {
    return gray_u && basis && inverse && !(elems_per_image % 12) && (gstride == 0 || gstride == elems_per_image / 3) && column >= 0xC0000000u;
}
inline mat3 mat3_of(const float* p) {
    mat3 r;
    for (int i = 0; i < 9; ++i) r.m[i] = p[i];
    return r;
}

// the x0 correction of a call: a known mode, a ratio in [0, 1] (a NaN fails both comparisons), a positive finite max_val and an image the
// largest kernel instantiation holds
inline bool x0fix_ok(int mode, double ratio, double max_val, int64_t elems_per_image) {
    return (mode == NATINF_X0_CLIP || mode == NATINF_X0_DYNAMIC) && ratio >= 0.0 && ratio <= 1.0 && max_val > 0.0 && max_val <= DBL_MAX &&
           elems_per_image <= 4 * (int64_t)kFixQuadsMax;
}
// where the quantile sits in the ascending |x0| of an image: rank = ratio*(n - 1) is ONE fp64 product; lo = floor(rank), hi = ceil(rank) is lo or
// lo + 1 (`next`), w = rank - lo (exact)
struct QuantilePos { unsigned lo; int next; double w; };
inline QuantilePos quantile_pos(double ratio, int64_t elems_per_image) {
    const double rank = ratio * (double)(elems_per_image - 1);
    const double lo = std::floor(rank);
    return QuantilePos{(unsigned)lo, std::ceil(rank) != lo, rank - lo};
}

// channels * height * width of a projection call, 0 when a factor is not positive or the product cannot be an image the kernels hold
inline int64_t project_elems(int channels, int height, int width) {
    constexpr int64_t cap = 4 * (int64_t)kFixQuadsMax;
    if (channels <= 0 || height <= 0 || width <= 0 || channels > cap || height > cap || width > cap) return 0;
    const int64_t n = (int64_t)channels * height * width;
    return n <= cap ? n : 0;
}
// the x0 projection of a call: `low` given, a scale of 2, 4 or 8 dividing height and width, an image of channels * height * width elements that
// is whole quads and fits the largest kernel instantiation, and a per-image stride of `low` that is 0 or the image's block count; fills g
inline bool project_ok(ProjGeom& g, const double* low, int channels, int height, int width, int scale, int64_t lstride, int64_t elems_per_image) {
    if (!low || (scale != 2 && scale != 4 && scale != 8)) return false;
    const int64_t n = project_elems(channels, height, width);
    if (!n || n != elems_per_image || (n & 3) || height % scale || width % scale) return false;
    if (lstride != 0 && lstride != n / (scale * scale)) return false;
    const int l2s = scale == 2 ? 1 : scale == 4 ? 2 : 3;
    g = ProjGeom{(int)(n / 4), l2s, width / scale, 1.0 / (double)(scale * scale)};
    return true;
}

// Host-side check of a small device int32 array before a launch (the noise row of natinf_step_f32prod_noise, the slots of
// natinf_step_f32prod_noise_guided and natinf_step_f16chain_guided): every one of the n values lies in lo..hi.  They are read back, kRowChunk at a time into
// one pinned buffer, on a private non-blocking stream of the current device: the host waits for those small copies only,
// never for the caller's stream.  1 = fine, 0 = a value outside the range, -1 = a HIP call failed.
constexpr int kRowChunk = 1024, kMaxDevices = 64;
inline int device_i32_in_range(const int32_t* p, int64_t n, int64_t lo, int64_t hi)
{
    static std::mutex mu;
    static hipStream_t streams[kMaxDevices] = {};
    static int32_t* bufs[kMaxDevices] = {};
    if (n == 0) return 1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) { (void)hipGetLastError(); return -1; }
    std::lock_guard<std::mutex> lock(mu);
    if (!streams[dev]) {
        hipStream_t s = nullptr;
        void* b = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return -1; }
        if (hipHostMalloc(&b, kRowChunk * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); (void)hipStreamDestroy(s); return -1;
        }
        streams[dev] = s; bufs[dev] = (int32_t*)b;
    }
    for (int64_t o = 0; o < n; o += kRowChunk) {
        const int c = n - o < kRowChunk ? (int)(n - o) : kRowChunk;
        if (hipMemcpyAsync(bufs[dev], p + o, c * sizeof(int32_t), hipMemcpyDefault, streams[dev]) != hipSuccess ||
            hipStreamSynchronize(streams[dev]) != hipSuccess) { (void)hipGetLastError(); return -1; }
        for (int i = 0; i < c; ++i)
            if (bufs[dev][i] < lo || bufs[dev][i] > hi) return 0;
    }
    return 1;
}

// a noise row: every column is in 0..k+1 (eps_j is drawn after step j-1) and column 0 has a `noise` to read
inline int noise_row_ok(const int32_t* idx_b, int n_b, int k, bool have_noise) {
    return device_i32_in_range(idx_b, n_b, have_noise ? 0 : 1, (int64_t)k + 1);
}
// a slot array: -1 (no unconditional row) or a row of `uncond`
inline int slots_ok(const int32_t* uncond_slot, int64_t n_images, int n_uncond) {
    return device_i32_in_range(uncond_slot, n_images, -1, (int64_t)n_uncond - 1);
}
// what an entry returns for a read-back's result: NATINF_OK (0) = go on, a value outside the range is the caller's fault, a failed HIP call the runtime's
inline int readback_code(int r) { return r > 0 ? NATINF_OK : (r < 0 ? NATINF_ELAUNCH : NATINF_EINVAL); }

}  // namespace

extern "C" {

int natinf_abi_version(void) { return NATINF_ABI_VERSION; }

const char* natinf_strerror(int code) {
    switch (code) {
        case NATINF_OK: return "ok";
        case NATINF_EINVAL: return "invalid argument";
        case NATINF_ELAUNCH: return "HIP launch failed";
        case NATINF_ENODEV: return "no gfx950 device or code object";
        case NATINF_ESTATE: return "handle in wrong state";
        default: return "unknown natinf error";
    }
}

int natinf_probe(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return NATINF_ENODEV; }
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&k_wsum_f64)) != hipSuccess) {
        (void)hipGetLastError();
        return NATINF_ENODEV;
    }
    return NATINF_OK;
}

int natinf_step_f64hist(const float* x_k, const float* model_out, const float* noise,
                        double* hist, float* x_next,
                        const int32_t* idx, const double* val, int n_terms, double c_diag,
                        int k, double alpha, double sigma, float std_f32, float b0_f32,
                        int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    if (!x_k || !model_out || !noise || !hist || !x_next || !terms_ok(idx, val, n_terms) || k < 0 || !nvec)
        return NATINF_EINVAL;
    hipLaunchKernelGGL(k_step_f64hist, dim3(grid_for(nvec)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)x_k, (const float4*)model_out, (const float4*)noise, hist, (float4*)x_next,
                       idx, val, n_terms, c_diag, k, alpha, sigma * sigma, std_f32, b0_f32, nvec, E);
    return launched();
}

int natinf_step_f32hist(const float* x_k, const float* model_out, const float* noise,
                        float* hist, float* x_next,
                        const int32_t* idx, const float* val, int n_terms, float c_diag,
                        int k, float alpha, float sigma, float std_f32, float b0_f32,
                        int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    if (!x_k || !model_out || !noise || !hist || !x_next || !terms_ok(idx, val, n_terms) || k < 0 || !nvec)
        return NATINF_EINVAL;
    hipLaunchKernelGGL(k_step_f32hist, dim3(grid_for(nvec)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)x_k, (const float4*)model_out, (const float4*)noise, hist, (float4*)x_next,
                       idx, val, n_terms, c_diag, k, 1.0f / alpha, sigma * sigma / std_f32, b0_f32, nvec, E);
    return launched();
}

int natinf_randn_philox_col_f32(float* out, int64_t n_images, int64_t elems_per_image, const int64_t* image_index,
                                int64_t first_index, int64_t index_stride, uint64_t seed, uint32_t column,
                                natinf_stream_t stream)
{
    const int64_t qpi = vec_count(elems_per_image, 4);
    if (!out || n_images <= 0 || !qpi) return NATINF_EINVAL;
    if (column && (qpi >> 32)) return NATINF_EINVAL;               // counter word 3 carries the column: the quad must fit word 2
    const int64_t total = qpi * n_images;
    hipLaunchKernelGGL(k_randn_philox, dim3(grid_for(total)), dim3(kBlock), 0, (hipStream_t)stream, (float4*)out,
                       image_index, first_index, index_stride, qpi, total, column, seed_lo(seed), seed_hi(seed));
    return launched();
}

int natinf_randn_philox_f32(float* out, int64_t n_images, int64_t elems_per_image, const int64_t* image_index,
                            int64_t first_index, int64_t index_stride, uint64_t seed, natinf_stream_t stream)
{
    return natinf_randn_philox_col_f32(out, n_images, elems_per_image, image_index, first_index, index_stride, seed, 0, stream);
}

int natinf_step_f64hist_noise(const float* x_k, const float* model_out, const float* noise,
                              double* hist, float* x_next,
                              const int32_t* idx, const double* val, int n_terms, double c_diag,
                              const int32_t* idx_b, const float* val_b, int n_b,
                              int k, double alpha, double sigma, float std_f32,
                              uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                              int64_t elems_per_image, int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    const unsigned blocks = quad_blocks(nvec);
    if (!step_f64_noise_ok(x_k, model_out, noise, hist, x_next, idx, val, n_terms, idx_b, val_b, n_b, k, nvec, elems_per_image, E) ||
        ((elems_per_image / 4) >> 32) || !blocks)
        return NATINF_EINVAL;
    // no read-back of the noise row here (natinf_step_f32prod_noise makes one): the caller keeps its columns in 0..k+1
    hipLaunchKernelGGL(k_step_noise_f64, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)x_k, (const float4*)model_out, (const float4*)noise, hist, (float4*)x_next,
                       idx, val, n_terms, c_diag, idx_b, val_b, n_b, image_index, first_index, index_stride,
                       elems_per_image / 4, seed_lo(seed), seed_hi(seed), k, alpha, sigma * sigma, std_f32, nvec, E);
    return launched();
}

int natinf_known_blend_f32(const float* x_in, float* out, const float* known, const uint8_t* mask,
                           int64_t known_image_stride, int64_t mask_image_stride,
                           float known_alpha_f32, float known_std_f32, uint32_t known_column,
                           uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                           int64_t elems_per_image, int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    const unsigned blocks = quad_blocks(nvec);
    if (!x_in || !out || !nvec || !image_ok(elems_per_image, E) || ((elems_per_image / 4) >> 32) || !blocks ||
        !known_ok(known, mask, known_image_stride, mask_image_stride, known_column, elems_per_image))
        return NATINF_EINVAL;
    hipLaunchKernelGGL(k_known_blend, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)x_in, (float4*)out, known, mask, known_image_stride, mask_image_stride,
                       known_alpha_f32, known_std_f32, known_column, image_index, first_index, index_stride,
                       elems_per_image / 4, seed_lo(seed), seed_hi(seed), nvec);
    return launched();
}

int natinf_step_f64hist_inpaint(const float* x_k, const float* model_out, const float* noise,
                                double* hist, float* x_next,
                                const int32_t* idx, const double* val, int n_terms, double c_diag,
                                const int32_t* idx_b, const float* val_b, int n_b,
                                int k, double alpha, double sigma, float std_f32,
                                uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                                int64_t elems_per_image, int64_t E,
                                const float* known, const uint8_t* mask, int64_t known_image_stride, int64_t mask_image_stride,
                                float known_alpha_f32, float known_std_f32, uint32_t known_column, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    const unsigned blocks = quad_blocks(nvec);
    if (!step_f64_noise_ok(x_k, model_out, noise, hist, x_next, idx, val, n_terms, idx_b, val_b, n_b, k, nvec, elems_per_image, E) ||
        ((elems_per_image / 4) >> 32) || !blocks ||
        !known_ok(known, mask, known_image_stride, mask_image_stride, known_column, elems_per_image))
        return NATINF_EINVAL;
    hipLaunchKernelGGL(k_step_inpaint_f64, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)x_k, (const float4*)model_out, (const float4*)noise, hist, (float4*)x_next,
                       idx, val, n_terms, c_diag, idx_b, val_b, n_b, image_index, first_index, index_stride,
                       elems_per_image / 4, seed_lo(seed), seed_hi(seed), k, alpha, sigma * sigma, std_f32,
                       known, mask, known_image_stride, mask_image_stride, known_alpha_f32, known_std_f32, known_column, nvec, E);
    return launched();
}

int natinf_x0_threshold_f64(double* x0, double* s_out, int64_t n_images, int64_t elems_per_image,
                            int mode, double ratio, double max_val, natinf_stream_t stream)
{
    const int64_t qpi = vec_count(elems_per_image, 4);
    if (!x0 || n_images <= 0 || n_images > INT32_MAX || !qpi || !x0fix_ok(mode, ratio, max_val, elems_per_image)) return NATINF_EINVAL;
    const QuantilePos p = quantile_pos(ratio, elems_per_image);
    auto kernel = qpi <= kFixQuadsSmall ? k_x0fix_f64<kFixQuadsSmall> : k_x0fix_f64<kFixQuadsMax>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_images), dim3(kBlock), 0, (hipStream_t)stream,
                       x0, s_out, (int)qpi, mode, p.lo, p.next, p.w, max_val);
    return launched();
}

int natinf_step_f64hist_x0fix(const float* x_k, const float* model_out, const float* noise,
                              double* hist, float* x_next,
                              const int32_t* idx, const double* val, int n_terms, double c_diag,
                              const int32_t* idx_b, const float* val_b, int n_b,
                              int k, double alpha, double sigma, float std_f32,
                              uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                              int64_t elems_per_image, int64_t E,
                              const float* known, const uint8_t* mask, int64_t known_image_stride, int64_t mask_image_stride,
                              float known_alpha_f32, float known_std_f32, uint32_t known_column,
                              int mode, double ratio, double max_val, double* s_out, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    if (!step_f64_noise_ok(x_k, model_out, noise, hist, x_next, idx, val, n_terms, idx_b, val_b, n_b, k, nvec, elems_per_image, E) ||
        !x0fix_ok(mode, ratio, max_val, elems_per_image) ||
        E / elems_per_image > INT32_MAX || (!known != !mask) ||
        (known && !known_ok(known, mask, known_image_stride, mask_image_stride, known_column, elems_per_image)))
        return NATINF_EINVAL;
    // no read-back of the noise row (natinf_step_f64hist_noise): every check above is a pure argument check, no device is touched
    const QuantilePos p = quantile_pos(ratio, elems_per_image);
    const int64_t qpi = elems_per_image / 4;
    auto kernel = qpi <= kFixQuadsSmall ? k_stepfix_f64<kFixQuadsSmall> : k_stepfix_f64<kFixQuadsMax>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(E / elems_per_image)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)x_k, (const float4*)model_out, (const float4*)noise, hist, (float4*)x_next,
                       idx, val, n_terms, c_diag, idx_b, val_b, n_b, image_index, first_index, index_stride,
                       (int)qpi, seed_lo(seed), seed_hi(seed), k, alpha, sigma * sigma, std_f32,
                       known, mask, known_image_stride, mask_image_stride, known_alpha_f32, known_std_f32, known_column,
                       mode, p.lo, p.next, p.w, max_val, s_out, E);
    return launched();
}

int natinf_x0_project_f64(double* x0, const double* low, double* r_out, int64_t n_images, int channels, int height, int width, int scale,
                          int64_t low_image_stride, natinf_stream_t stream)
{
    const int64_t elems_per_image = project_elems(channels, height, width);
    ProjGeom g;
    if (!x0 || n_images <= 0 || n_images > INT32_MAX ||
        !project_ok(g, low, channels, height, width, scale, low_image_stride, elems_per_image))
        return NATINF_EINVAL;
    auto kernel = g.qpi <= kFixQuadsSmall ? k_x0project_f64<kFixQuadsSmall> : k_x0project_f64<kFixQuadsMax>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_images), dim3(kBlock), 0, (hipStream_t)stream, x0, low, r_out, low_image_stride, g);
    return launched();
}

int natinf_step_f64hist_project(const float* x_k, const float* model_out, const float* noise,
                                double* hist, float* x_next,
                                const int32_t* idx, const double* val, int n_terms, double c_diag,
                                const int32_t* idx_b, const float* val_b, int n_b,
                                int k, double alpha, double sigma, float std_f32,
                                uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                                int64_t elems_per_image, int64_t E,
                                const double* low, int64_t low_image_stride, int channels, int height, int width, int scale,
                                double* r_out, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    ProjGeom g;
    if (!step_f64_noise_ok(x_k, model_out, noise, hist, x_next, idx, val, n_terms, idx_b, val_b, n_b, k, nvec, elems_per_image, E) ||
        !quad_blocks(nvec) || E / elems_per_image > INT32_MAX ||
        !project_ok(g, low, channels, height, width, scale, low_image_stride, elems_per_image))
        return NATINF_EINVAL;
    // no read-back of the noise row (natinf_step_f64hist_noise): every check above is a pure argument check, no device is touched
    auto kernel = g.qpi <= kFixQuadsSmall ? k_stepproject_f64<kFixQuadsSmall> : k_stepproject_f64<kFixQuadsMax>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(E / elems_per_image)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)x_k, (const float4*)model_out, (const float4*)noise, hist, (float4*)x_next,
                       idx, val, n_terms, c_diag, idx_b, val_b, n_b, image_index, first_index, index_stride,
                       seed_lo(seed), seed_hi(seed), k, alpha, sigma * sigma, std_f32,
                       low, low_image_stride, g, r_out, E);
    return launched();
}

int natinf_color_blend_f32(const float* x_in, float* out, const float* gray_u, int64_t gray_image_stride,
                           const float basis[9], const float inverse[9],
                           float gray_alpha_f32, float gray_std_f32, uint32_t gray_column,
                           uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                           int64_t elems_per_image, int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    if (!x_in || !out || !nvec || !image_ok(elems_per_image, E) || ((elems_per_image / 4) >> 32) ||
        !gray_ok(gray_u, basis, inverse, gray_image_stride, gray_column, elems_per_image))
        return NATINF_EINVAL;
    const int64_t npq = nvec / 3;                                   // pixel quads: one thread each
    const unsigned blocks = quad_blocks(npq);
    if (!blocks) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_color_blend, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)x_in, (float4*)out, gray_u, gray_image_stride, mat3_of(basis), mat3_of(inverse),
                       gray_alpha_f32, gray_std_f32, gray_column, image_index, first_index, index_stride,
                       elems_per_image / 12, seed_lo(seed), seed_hi(seed), npq);
    return launched();
}

int natinf_step_f64hist_colorize(const float* x_k, const float* model_out, const float* noise,
                                 double* hist, float* x_next,
                                 const int32_t* idx, const double* val, int n_terms, double c_diag,
                                 const int32_t* idx_b, const float* val_b, int n_b,
                                 int k, double alpha, double sigma, float std_f32,
                                 uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                                 int64_t elems_per_image, int64_t E,
                                 const float* gray_u, int64_t gray_image_stride, const float basis[9], const float inverse[9],
                                 float gray_alpha_f32, float gray_std_f32, uint32_t gray_column, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    if (!step_f64_noise_ok(x_k, model_out, noise, hist, x_next, idx, val, n_terms, idx_b, val_b, n_b, k, nvec, elems_per_image, E) ||
        ((elems_per_image / 4) >> 32) || !quad_blocks(nvec) ||
        !gray_ok(gray_u, basis, inverse, gray_image_stride, gray_column, elems_per_image))
        return NATINF_EINVAL;
    const int64_t npq = nvec / 3;                                   // pixel quads: one thread each
    hipLaunchKernelGGL(k_step_colorize_f64, dim3(quad_blocks(npq)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)x_k, (const float4*)model_out, (const float4*)noise, hist, (float4*)x_next,
                       idx, val, n_terms, c_diag, idx_b, val_b, n_b, image_index, first_index, index_stride,
                       elems_per_image / 12, seed_lo(seed), seed_hi(seed), k, alpha, sigma * sigma, std_f32,
                       gray_u, gray_image_stride, mat3_of(basis), mat3_of(inverse), gray_alpha_f32, gray_std_f32, gray_column, npq, E);
    return launched();
}

int natinf_weighted_sum_f64(const double* hist, float* out, const int32_t* idx, const double* val, int n_terms,
                            int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    if (!hist || !out || !terms_ok(idx, val, n_terms) || !nvec) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_wsum_f64, dim3(grid_for(nvec)), dim3(kBlock), 0, (hipStream_t)stream,
                       hist, (float4*)out, idx, val, n_terms, nvec, E);
    return launched();
}

int natinf_to_pixel_u8(const float* x, uint8_t* out, int B, int C, int H, int W, int centered, natinf_stream_t stream)
{
    if (!x || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0) return NATINF_EINVAL;
    if ((int64_t)C * H * W > (1 << 30) || B > 65535) return NATINF_EINVAL;
    const int per = C * H * W;
    int gx = (per + kBlock - 1) / kBlock;
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(k_to_pixel, dim3(gx, B), dim3(kBlock), 0, (hipStream_t)stream, x, out, C, H * W, centered);
    return launched();
}

int natinf_step_f32prod(const float* z, const float* cond, const float* uncond, float cfg,
                        int64_t sample_elems, int64_t eps_sample_stride,
                        float* hist_x0, const float* hist_eps, float* z_next,
                        const int32_t* idx_c, const float* val_c, int n_c, float c_diag,
                        const int32_t* idx_b, const float* val_b, int n_b,
                        int k, float c1_f32, float c2_f32, int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    if (!z || !cond || !hist_x0 || !hist_eps || !z_next || !terms_ok(idx_c, val_c, n_c) || !terms_ok(idx_b, val_b, n_b) ||
        k < 0 || !nvec || !image_ok(sample_elems, E) || eps_sample_stride < sample_elems || (eps_sample_stride & 3))
        return NATINF_EINVAL;
    hipLaunchKernelGGL(k_step_f32prod, dim3(grid_for(nvec)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)z, cond, uncond, cfg, sample_elems / 4, eps_sample_stride,
                       hist_x0, hist_eps, (float4*)z_next, idx_c, val_c, n_c, c_diag, idx_b, val_b, n_b,
                       k, c1_f32, c2_f32, nvec, E);
    return launched();
}

int natinf_step_f32prod_noise(const float* z, const float* cond, const float* uncond, float cfg,
                              int64_t sample_elems, int64_t eps_sample_stride,
                              float* hist_x0, const float* noise, float* z_next,
                              const int32_t* idx_c, const float* val_c, int n_c, float c_diag,
                              const int32_t* idx_b, const float* val_b, int n_b,
                              int k, float c1_f32, float c2_f32,
                              uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                              int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    const unsigned blocks = quad_blocks(nvec);
    if (!step_f32prod_seeded_ok(z, cond, hist_x0, z_next, idx_c, val_c, n_c, idx_b, val_b, n_b, k, nvec, blocks, sample_elems, eps_sample_stride, E))
        return NATINF_EINVAL;
    if (const int rc = readback_code(noise_row_ok(idx_b, n_b, k, noise != nullptr))) return rc;
    hipLaunchKernelGGL(k_step_noise_f32prod, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)z, cond, uncond, cfg, sample_elems / 4, eps_sample_stride,
                       hist_x0, (const float4*)noise, (float4*)z_next, idx_c, val_c, n_c, c_diag, idx_b, val_b, n_b,
                       image_index, first_index, index_stride, seed_lo(seed), seed_hi(seed),
                       k, c1_f32, c2_f32, nvec, E);
    return launched();
}

int natinf_step_f32prod_noise_guided(const float* z, const float* cond, const float* uncond,
                                     const float* cfg_image, const int32_t* uncond_slot, int n_uncond,
                                     int64_t sample_elems, int64_t eps_sample_stride,
                                     float* hist_x0, const float* noise, float* z_next,
                                     const int32_t* idx_c, const float* val_c, int n_c, float c_diag,
                                     const int32_t* idx_b, const float* val_b, int n_b,
                                     int k, float c1_f32, float c2_f32,
                                     uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                                     int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    const unsigned blocks = quad_blocks(nvec);
    if (!step_f32prod_seeded_ok(z, cond, hist_x0, z_next, idx_c, val_c, n_c, idx_b, val_b, n_b, k, nvec, blocks, sample_elems, eps_sample_stride, E) ||
        !guidance_ok(cfg_image, uncond_slot, n_uncond, uncond))
        return NATINF_EINVAL;
    if (const int rc = readback_code(noise_row_ok(idx_b, n_b, k, noise != nullptr))) return rc;
    if (const int rc = readback_code(slots_ok(uncond_slot, E / sample_elems, n_uncond))) return rc;
    hipLaunchKernelGGL(k_step_guided_f32prod, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)z, cond, uncond, cfg_image, uncond_slot, sample_elems / 4, eps_sample_stride,
                       hist_x0, (const float4*)noise, (float4*)z_next, idx_c, val_c, n_c, c_diag, idx_b, val_b, n_b,
                       image_index, first_index, index_stride, seed_lo(seed), seed_hi(seed),
                       k, c1_f32, c2_f32, nvec, E);
    return launched();
}

int natinf_step_f32prod_inpaint(const float* z, const float* cond, const float* uncond,
                                const float* cfg_image, const int32_t* uncond_slot, int n_uncond,
                                int64_t sample_elems, int64_t eps_sample_stride,
                                float* hist_x0, const float* noise, float* z_next,
                                const int32_t* idx_c, const float* val_c, int n_c, float c_diag,
                                const int32_t* idx_b, const float* val_b, int n_b,
                                int k, float c1_f32, float c2_f32,
                                uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                                int64_t E,
                                const float* known, const uint8_t* mask, int64_t known_image_stride, int64_t mask_image_stride,
                                float known_alpha_f32, float known_std_f32, uint32_t known_column, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    const unsigned blocks = quad_blocks(nvec);
    // every pure argument check, the blend's included, before the first read-back: a refusal of these touches no device
    if (!step_f32prod_seeded_ok(z, cond, hist_x0, z_next, idx_c, val_c, n_c, idx_b, val_b, n_b, k, nvec, blocks, sample_elems, eps_sample_stride, E) ||
        !guidance_ok(cfg_image, uncond_slot, n_uncond, uncond) ||
        !known_ok(known, mask, known_image_stride, mask_image_stride, known_column, sample_elems))
        return NATINF_EINVAL;
    if (const int rc = readback_code(noise_row_ok(idx_b, n_b, k, noise != nullptr))) return rc;
    if (const int rc = readback_code(slots_ok(uncond_slot, E / sample_elems, n_uncond))) return rc;
    hipLaunchKernelGGL(k_step_inpaint_f32prod, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)z, cond, uncond, cfg_image, uncond_slot, sample_elems / 4, eps_sample_stride,
                       hist_x0, (const float4*)noise, (float4*)z_next, idx_c, val_c, n_c, c_diag, idx_b, val_b, n_b,
                       image_index, first_index, index_stride, seed_lo(seed), seed_hi(seed),
                       k, c1_f32, c2_f32, known, mask, known_image_stride, mask_image_stride,
                       known_alpha_f32, known_std_f32, known_column, nvec, E);
    return launched();
}

int natinf_weighted_sum_f32prod(const float* hist, float* out, const int32_t* idx, const float* val, int n_terms,
                                int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 4);
    if (!hist || !out || !terms_ok(idx, val, n_terms) || !nvec) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_wsum_f32prod, dim3(grid_for(nvec)), dim3(kBlock), 0, (hipStream_t)stream,
                       hist, (float4*)out, idx, val, n_terms, nvec, E);
    return launched();
}

int natinf_step_f16chain(const void* x, const void* v_text, const void* v_null, const void* noise,
                         void* hist, void* mean_out, void* x_next,
                         const int32_t* idx, const float* val, int n_terms, float c_diag, float w_total,
                         int k, float sig, float sig_next, float one_minus_sig_next, float cfg,
                         int flags, int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 8);
    if (!x || !v_text || !v_null || !hist || !terms_ok(idx, val, n_terms) || k < 0 || !nvec ||
        (x_next && !noise) || (flags & ~NATINF_SD3_CFG_ON_VELOCITY))
        return NATINF_EINVAL;
    const auto kern = (flags & NATINF_SD3_CFG_ON_VELOCITY) ? k_step_f16chain<true> : k_step_f16chain<false>;
    hipLaunchKernelGGL(kern, dim3(grid_for(nvec)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const h8*)x, (const h8*)v_text, (const h8*)v_null, (const h8*)noise, (h16*)hist,
                       (h8*)mean_out, (h8*)x_next, idx, val, n_terms, c_diag, w_total, k, sig, sig_next,
                       one_minus_sig_next, cfg, nvec, E);
    return launched();
}

int natinf_step_f16chain_guided(const void* x, const void* v_text, const void* v_null,
                                const float* cfg_image, const int32_t* uncond_slot, int n_uncond, int64_t sample_elems,
                                const void* noise, void* hist, void* mean_out, void* x_next,
                                const int32_t* idx, const float* val, int n_terms, float c_diag, float w_total,
                                int k, float sig, float sig_next, float one_minus_sig_next,
                                int flags, int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 8);
    if (!x || !v_text || !hist || !terms_ok(idx, val, n_terms) || k < 0 || !nvec ||
        (x_next && !noise) || (flags & ~NATINF_SD3_CFG_ON_VELOCITY) || !image_ok(sample_elems, E, 8) ||
        !guidance_ok(cfg_image, uncond_slot, n_uncond, v_null))
        return NATINF_EINVAL;
    if (const int rc = readback_code(slots_ok(uncond_slot, E / sample_elems, n_uncond))) return rc;
    const auto kern = (flags & NATINF_SD3_CFG_ON_VELOCITY) ? k_step_f16chain_guided<true> : k_step_f16chain_guided<false>;
    hipLaunchKernelGGL(kern, dim3(grid_for(nvec)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const h8*)x, (const h8*)v_text, (const h8*)v_null, cfg_image, uncond_slot, sample_elems / 8,
                       (const h8*)noise, (h16*)hist, (h8*)mean_out, (h8*)x_next, idx, val, n_terms, c_diag, w_total,
                       k, sig, sig_next, one_minus_sig_next, nvec, E);
    return launched();
}

int natinf_known_blend_f16(const void* x_in, void* out, const void* noise, const void* known, const uint8_t* mask,
                           int64_t known_image_stride, int64_t mask_image_stride,
                           float sig, float one_minus_sig, uint32_t known_column, uint64_t seed,
                           const int64_t* image_index, int64_t first_index, int64_t index_stride,
                           int64_t elems_per_image, int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 8);
    const unsigned blocks = quad_blocks(nvec);
    if (!x_in || !out || !nvec || !image_ok(elems_per_image, E, 8) || !blocks ||
        !known_ok_f16(known, mask, known_image_stride, mask_image_stride, known_column, elems_per_image, noise != nullptr))
        return NATINF_EINVAL;
    hipLaunchKernelGGL(k_blend_known_f16, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       (const h8*)x_in, (h8*)out, (const h8*)noise, (const h8*)known, mask, known_image_stride, mask_image_stride,
                       sig, one_minus_sig, known_column, image_index, first_index, index_stride, elems_per_image / 8,
                       seed_lo(seed), seed_hi(seed), nvec);
    return launched();
}

int natinf_step_f16chain_inpaint(const void* x, const void* v_text, const void* v_null,
                                 const float* cfg_image, const int32_t* uncond_slot, int n_uncond, int64_t sample_elems,
                                 const void* noise, void* hist, void* mean_out, void* x_next,
                                 const int32_t* idx, const float* val, int n_terms, float c_diag, float w_total,
                                 int k, float sig, float sig_next, float one_minus_sig_next,
                                 int flags, int64_t E,
                                 const void* known, const uint8_t* mask, int64_t known_image_stride, int64_t mask_image_stride,
                                 uint32_t known_column, uint64_t seed,
                                 const int64_t* image_index, int64_t first_index, int64_t index_stride, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 8);
    const unsigned blocks = quad_blocks(nvec);
    // every pure argument check, the blend's included, before the slot read-back: a refusal of these touches no device
    if (!x || !v_text || !hist || !terms_ok(idx, val, n_terms) || k < 0 || !nvec || !blocks ||
        (x_next && !noise) || (flags & ~(NATINF_SD3_CFG_ON_VELOCITY | NATINF_SD3_BLEND_MEAN)) || !image_ok(sample_elems, E, 8) ||
        !guidance_ok(cfg_image, uncond_slot, n_uncond, v_null) ||
        !known_ok_f16(known, mask, known_image_stride, mask_image_stride, known_column, sample_elems, noise != nullptr || !x_next))
        return NATINF_EINVAL;
    if (const int rc = readback_code(slots_ok(uncond_slot, E / sample_elems, n_uncond))) return rc;
    const auto kern = (flags & NATINF_SD3_CFG_ON_VELOCITY) ? k_step_inpaint_f16chain<true> : k_step_inpaint_f16chain<false>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       (const h8*)x, (const h8*)v_text, (const h8*)v_null, cfg_image, uncond_slot, sample_elems / 8,
                       (const h8*)noise, (h16*)hist, (h8*)mean_out, (h8*)x_next, idx, val, n_terms, c_diag, w_total,
                       k, sig, sig_next, one_minus_sig_next,
                       (const h8*)known, mask, known_image_stride, mask_image_stride, known_column, (flags & NATINF_SD3_BLEND_MEAN) != 0,
                       image_index, first_index, index_stride, seed_lo(seed), seed_hi(seed), nvec, E);
    return launched();
}

int natinf_flow_input_f16(const void* noise, const void* mean, void* out, float sig, float one_minus_sig,
                          int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 8);
    if (!noise || !out || !nvec) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_flow_input_f16, dim3(grid_for(nvec)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const h8*)noise, (const h8*)mean, (h8*)out, sig, one_minus_sig, nvec);
    return launched();
}

int natinf_weighted_mean_f16(const void* hist, void* out, const int32_t* idx, const float* val, int n_terms,
                             float w_total, int64_t E, natinf_stream_t stream)
{
    const int64_t nvec = vec_count(E, 8);
    if (!hist || !out || !terms_ok(idx, val, n_terms) || !nvec) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_wmean_f16, dim3(grid_for(nvec)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const h16*)hist, (h8*)out, idx, val, n_terms, w_total, nvec, E);
    return launched();
}

int natinf_vae_posterior_f32(const float* moments, float* latents, int64_t n_images, int latent_ch, int64_t hw,
                             int sample, float scale, float shift,
                             uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                             natinf_stream_t stream)
{
    if (!moments || !latents || n_images < 1 || latent_ch < 1 || hw < 1 || hw > (INT64_MAX >> 1) / latent_ch) return NATINF_EINVAL;
    const int64_t qpi = vec_count((int64_t)latent_ch * hw, 4);
    if (!qpi || (qpi >> 32) || n_images > INT64_MAX / (2 * qpi)) return NATINF_EINVAL;      // counter word 3 carries the column: the quad must fit word 2
    const int64_t nvec = qpi * n_images;
    const unsigned blocks = quad_blocks(nvec);
    if (!blocks) return NATINF_EINVAL;
    hipLaunchKernelGGL(k_vae_posterior, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, (const float4*)moments, (float4*)latents,
                       sample != 0, scale, shift, image_index, first_index, index_stride, qpi, seed_lo(seed), seed_hi(seed), nvec);
    return launched();
}

int natinf_posterior_samples(const void* feats_bf16, const float* noise_or_null, float a, float b,
                             uint64_t seed, const int64_t* index, int64_t first_index, int64_t index_stride,
                             int n, int d, void* workspace, natinf_stream_t stream)
{
    if (!feats_bf16 || !workspace || !post::shape_ok(n, d)) return NATINF_EINVAL;
    if (((uintptr_t)feats_bf16 & 15) || ((uintptr_t)noise_or_null & 15) || ((uintptr_t)workspace & 255)) return NATINF_EINVAL;
    const post::Layout L = post::layout(n, d);
    const int d8 = d / 8;
    hipLaunchKernelGGL(k_post_samples, dim3((d8 + kBlock - 1) / kBlock, n), dim3(kBlock), 0, (hipStream_t)stream,
                       (const bf16x8*)feats_bf16, (const float4*)noise_or_null, a, b, index, first_index, index_stride,
                       seed_lo(seed), seed_hi(seed), d8, (int64_t)n * d8,
                       reinterpret_cast<bf16x8*>(static_cast<unsigned char*>(workspace) + L.planes));
    return launched();
}

}  // extern "C"
