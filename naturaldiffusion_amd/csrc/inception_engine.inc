// inception_engine.inc -- FID Inception-V3 pool3 engine (C ABI of include/natinf_inception.h); included after vae_engine.inc.
//
// Replaces `InceptionV3([block_idx])(batch)[0]` of the reference's FID epilogue (src/CIFAR10NaturalInference.py:44-86).  The module
// comes from un-vendored pytorch_fid / torchvision; include/natinf_inception.h states the parity status of that third-party arithmetic
// (PARITY UNPINNED) and what the engine is tested against.  Design: the FID epilogue is < 0.1 % of a 50k-image run's flops (5.7 GFLOP per image against 325 GFLOP of
// sampling) -- but 20 % of the WALL time of config 3's job on this library's generator (round 4), hence the round-5 rebuild.  Three plans (natinf_set_inception_conv):
//   * NHWC 16-bit activations; every Mixed_* block writes its branches straight into the channel slices of one concat buffer;
//   * BatchNorm (eval) is folded into the filter rows and an fp32 bias when the weights are packed; ReLU is the convolution's epilogue;
//   * plans 0 / 1 (bf16): the folded filters are kept as TWO bf16 terms, W = W_hi + W_lo (W_lo = the rounding residual of W_hi), multiplied as two passes over the
//     SAME activation operand: a bf16-rounded filter is off by the same amount for every image, so its error does not average out over a data set -- it shifts
//     the feature MEANS, which is exactly what a Frechet distance measures (measured on 2,000 images: |d mu|^2 = 0.095 of a Frechet distance of 0.099 with
//     single-term filters);
//   * plan 2 (the default): IEEE-half activations and ONE half-precision filter term per power-of-two-scaled row (k_inc_pack_f16; conv_ring.h has the argument
//     and the measured statistics): eleven significant bits do for the means what the second bf16 term did, at half the matrix work;
//   * round 5: every convolution behind the stem is ONE launch of k_conv_ring (conv_ring.h): an implicit GEMM whose A operand is the activation tensor itself -- a
//     K-tile is one tap x 32 channels, fetched by LDS-DMA at the tap's shift, padding taps from a page of zeros.  Channel counts that are no multiple of 32
//     (48, 80) are padded by their producer (zero filter rows: the pad channels hold relu(0) = 0).  Before: k_inc_im2col + one LDS-DMA GEMM per convolution
//     (natinf_set_inception_conv(0) still runs that plan: A/B runs and the parity test between the two); the copy kernel alone was 30 % of a forward of 500 images;
//   * the stem fuses /255, the 299x299 bilinear resize (align_corners = False), 2x - 1 and the patch rows of Conv2d_1a_3x3 in one kernel;
//   * 3x3 max / average pools (count_include_pad = False, the FID variant): row walkers (k_inc_pool); the final 8x8 average is a small bandwidth kernel.
#include "natinf_inception.h"
#include "engine_core.h"
#include "conv_ring.h"

namespace ncsn {

// stem: u8 [B][H][W][3] or f32 [B][3][H][W] in [0, 1]  ->  rows of the Conv2d_1a_3x3 im2col matrix [B*149*149][64] (k = (ky*3 + kx)*3 + c; 27..63 zero)
// F.interpolate(size = 299, mode = 'bilinear', align_corners = False): src = max(0, (dst + 0.5) * in / out - 0.5)
// 16-bit activations of the engine: bf16 (plans 0 / 1) or IEEE half (plan 2)
__device__ __forceinline__ unsigned short inc_cvt16(float v, int f16) {
    if (f16) { const _Float16 h = (_Float16)fminf(fmaxf(v, -65504.f), 65504.f); return __builtin_bit_cast(unsigned short, h); }      // saturating, as conv_ring_epilogue
    const bf16 h = (bf16)v; return __builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float inc_f32(unsigned short u, int f16) {
    if (f16) return (float)__builtin_bit_cast(_Float16, u);
    return __uint_as_float((unsigned)u << 16);
}
// (lg_slots: 4 = rows of 64 columns -- the GEMM of plans 0 / 1 wants 64-wide K-tiles --, 3 = rows of 32: k_conv_ring's K-tile, half the bytes)
// Round 6: blockIdx.y = (sample, output row), threads over (output column, 4-column slot).  The four source rows an output row can touch (bilinear taps of image rows
// 2 oy .. 2 oy + 2 of the 299 x 299 image) are staged in LDS once per block as the fp32 values the first form computed per tap (u8 / 255: the reference's true division;
// fp32 input: the value itself), and an element's four taps are LDS reads: the first form issued sixteen scattered BYTE loads per thread, and the CU's one address unit
// -- not memory -- bound it at 0.95 ms per 500 images (0.75 TB/s of stores).  Same arithmetic per element: same bytes.  W <= STEM_WMAX (CIFAR10: 32); wider inputs take
// the direct loads.
constexpr int STEM_WMAX = 128;
__global__ __launch_bounds__(256) void k_inc_stem(const void* __restrict__ img, int is_u8, int H, int W, unsigned short* __restrict__ out, int B, int f16, int lg_slots)
{
    __shared__ float srow[4][STEM_WMAX * 3];
    const unsigned by = blockIdx.y, b = by / 149u, oy = by - b * 149u;
    const float sy = (float)H / 299.0f, sx = (float)W / 299.0f;
    float fy_lo = ((float)(oy * 2u) + 0.5f) * sy - 0.5f;
    fy_lo = fy_lo < 0.f ? 0.f : fy_lo;
    const int r_lo = (int)fy_lo;                                             // first source row of this output row's taps; the last one is <= r_lo + 3 (sy <= 1 ... any sy: checked below)
    const bool staged = W <= STEM_WMAX;
    if (staged) {
        for (int t = threadIdx.x; t < 4 * W * 3; t += 256) {
            const int j = t / (W * 3), xc = t - j * (W * 3), x = xc / 3, c = xc - x * 3, y = min(r_lo + j, H - 1);
            float v;
            if (is_u8) v = (float)reinterpret_cast<const unsigned char*>(img)[((int64_t)b * H + y) * W * 3 + xc] / 255.0f;
            else v = reinterpret_cast<const float*>(img)[(((int64_t)b * 3 + c) * H + y) * W + x];
            srow[j][xc] = v;
        }
        __syncthreads();
    }
    const unsigned t = blockIdx.x * 256u + threadIdx.x;                        // (output column, slot of four columns of the patch row)
    const unsigned ox = t >> lg_slots, slot = t & ((1u << lg_slots) - 1u);
    if (ox >= 149u) return;
    const int64_t row = (int64_t)by * 149 + ox;
    unsigned short* dst = out + ((row << lg_slots) + slot) * 4;
    unsigned short o4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = (int)slot * 4 + e;
        float v = 0.f;
        if (k < 27) {
            const int tap = k / 3, c = k - tap * 3, ky = tap / 3, kx = tap - ky * 3;
            const int y = (int)oy * 2 + ky, x = (int)ox * 2 + kx;                // pixel of the 299 x 299 image (stride 2, no padding)
            float fy = ((float)y + 0.5f) * sy - 0.5f, fx = ((float)x + 0.5f) * sx - 0.5f;
            fy = fy < 0.f ? 0.f : fy; fx = fx < 0.f ? 0.f : fx;
            const int y0 = (int)fy, x0 = (int)fx;
            const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
            const float ly = fy - (float)y0, lx = fx - (float)x0;
            float p00, p01, p10, p11;
            if (staged && y1 - r_lo <= 3) {                                      // (always, for H <= 299: three image rows span less than one source row step + 1)
                const int j0 = y0 - r_lo, j1 = y1 - r_lo;
                p00 = srow[j0][x0 * 3 + c]; p01 = srow[j0][x1 * 3 + c]; p10 = srow[j1][x0 * 3 + c]; p11 = srow[j1][x1 * 3 + c];
            } else if (is_u8) {
                const unsigned char* s = reinterpret_cast<const unsigned char*>(img) + (int64_t)b * H * W * 3;
                // the reference divides the uint8 tensor by 255 (a true fp32 division)
                p00 = (float)s[(y0 * W + x0) * 3 + c] / 255.0f; p01 = (float)s[(y0 * W + x1) * 3 + c] / 255.0f;
                p10 = (float)s[(y1 * W + x0) * 3 + c] / 255.0f; p11 = (float)s[(y1 * W + x1) * 3 + c] / 255.0f;
            } else {
                const float* s = reinterpret_cast<const float*>(img) + ((int64_t)b * 3 + c) * H * W;
                p00 = s[y0 * W + x0]; p01 = s[y0 * W + x1]; p10 = s[y1 * W + x0]; p11 = s[y1 * W + x1];
            }
            const float r = (1.0f - ly) * ((1.0f - lx) * p00 + lx * p01) + ly * ((1.0f - lx) * p10 + lx * p11);
            v = 2.0f * r - 1.0f;
        }
        o4[e] = inc_cvt16(v, f16);
    }
    *reinterpret_cast<uint2*>(dst) = make_uint2((unsigned)o4[0] | ((unsigned)o4[1] << 16), (unsigned)o4[2] | ((unsigned)o4[3] << 16));
}

// (k_inc_im2col, the generic im2col pass: ncsnpp_kernels.h -- the `ddpm` plan's stride-2 Downsample convolution uses it too)

// 3x3 pool, stride s, padding p: mode 0 = max (padding never wins), 1 = average over the VALID elements (count_include_pad = False)
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
// Round 5: one thread per (sample, output row, 8-channel chunk) WALKS the row -- every input column is reduced over its (up to) three rows once and kept in
// registers for the next output(s): three 16-byte loads per output at stride 1 (six at stride 2) instead of nine, no per-output index arithmetic (the old form
// decoded its pixel with three 64-bit divisions per thread).  MODE 0 = max (padding never wins), 1 = average over the VALID elements (count_include_pad = False).
// Round 6: every load is UNCONDITIONAL (row / column clamped into the image, the value dropped afterwards) and the next output's new column(s) are requested before the
// current ones are reduced.  The first form guarded each load with its row's validity -- a per-lane branch the compiler cannot hoist a load across -- so a thread paid
// three dependent memory round trips per output (105 per row of 35): 290-420 us per launch at ~1 TB/s.  Same sums in the same order: same bytes.
template <int F16, int MODE, int STRIDE>
__global__ __launch_bounds__(256) void k_inc_pool(const unsigned short* __restrict__ x, int H, int W, int ld, int C, int pad, int Ho, int Wo,
                                                  unsigned short* __restrict__ out, int ld_out, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned cc = (unsigned)C >> 3, chunk = i % cc, row = i / cc, oy = row % (unsigned)Ho, b = row / (unsigned)Ho;
    const int y0 = (int)oy * STRIDE - pad;
    const unsigned short* xb = x + ((int64_t)b * H) * W * ld + chunk * 8;
    bool rv[3]; int nvr = 0; int64_t ro[3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) { rv[ky] = (unsigned)(y0 + ky) < (unsigned)H; nvr += rv[ky]; ro[ky] = (int64_t)min(max(y0 + ky, 0), H - 1) * W; }
    struct Col { u16x8 v[3]; };
    auto fetch = [&](int xx) __attribute__((always_inline)) {
        Col c_;
        const int xc = min(max(xx, 0), W - 1);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) c_.v[ky] = *reinterpret_cast<const u16x8*>(xb + (ro[ky] + xc) * ld);
        return c_;
    };
    auto reduce = [&](int xx, const Col& c_, float (&r)[8]) __attribute__((always_inline)) {
        const bool cv = (unsigned)xx < (unsigned)W;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = MODE == 0 ? -INFINITY : 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const bool ok = cv && rv[ky];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = inc_f32(c_.v[ky][e], F16);
                r[e] = MODE == 0 ? fmaxf(r[e], ok ? f : -INFINITY) : r[e] + (ok ? f : 0.f);       // (x + 0 = x, max(x, -inf) = x: the skipped term of the first form)
            }
        }
    };
    float ca[8], cb[8], cn[8];
    { const Col a0 = fetch(-pad), a1 = fetch(1 - pad); reduce(-pad, a0, ca); reduce(1 - pad, a1, cb); }
    unsigned short* o = out + ((int64_t)row * Wo) * ld_out + chunk * 8;
    Col nx = fetch(2 - pad), nx2;
    if constexpr (STRIDE == 2) nx2 = fetch(3 - pad);
    for (int ox = 0; ox < Wo; ++ox) {
        const int x0 = ox * STRIDE - pad;
        const Col cur = nx;
        Col cur2;
        if constexpr (STRIDE == 2) cur2 = nx2;
        nx = fetch(x0 + STRIDE + 2);                                        // the next output's columns: in flight while this output is reduced and stored
        if constexpr (STRIDE == 2) nx2 = fetch(x0 + STRIDE + 3);
        reduce(x0 + 2, cur, cn);
        float inv = 1.0f;
        if constexpr (MODE == 1) {
            const int nvc = ((unsigned)x0 < (unsigned)W) + ((unsigned)(x0 + 1) < (unsigned)W) + ((unsigned)(x0 + 2) < (unsigned)W);
            inv = 1.0f / (float)(nvr * nvc);
        }
        u16x8 ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) ov[e] = inc_cvt16(MODE == 0 ? fmaxf(fmaxf(ca[e], cb[e]), cn[e]) : ((ca[e] + cb[e]) + cn[e]) * inv, F16);
        *reinterpret_cast<u16x8*>(o + (int64_t)ox * ld_out) = ov;
        if constexpr (STRIDE == 1) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { ca[e] = cb[e]; cb[e] = cn[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) ca[e] = cn[e];
            reduce(x0 + 3, cur2, cb);
        }
    }
}

// adaptive_avg_pool2d(., (1, 1)): x [B][HW][C] bf16 -> out [B][C] fp32
__global__ __launch_bounds__(256) void k_inc_global_avg(const unsigned short* __restrict__ x, int HW, int C, float* __restrict__ out, int64_t total, int f16)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C); const int64_t b = i / C;
    float s = 0.f;
    for (int p = 0; p < HW; ++p) s += inc_f32(x[((int64_t)b * HW + p) * C + c], f16);
    out[i] = s / (float)HW;
}

// BasicConv2d = conv (no bias) -> BatchNorm(eval, eps 1e-3) -> ReLU, folded: W'[n][k] = W[n][c][ky][kx] * g[n] / sqrt(var[n] + eps) with
// k = (ky*kw + kx)*C + c (zero for k >= K);  b'[n] = beta[n] - mean[n] * g[n] / sqrt(var[n] + eps).
// wp [N][2 * Kp]: columns [0, Kp) = bf16(W'), columns [Kp, 2 Kp) = bf16(W' - float(bf16(W')))
// Cp >= C: channels per tap in the packed K order (k = tap * Cp + c; the implicit-GEMM plan pads 48 / 80 input channels to 64 / 96: zero columns);
// Np >= N: packed filter rows (rows N .. Np-1 and their bias are zero: the pad channels of the OUTPUT tensor)
__global__ __launch_bounds__(256) void k_inc_pack(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  const float* __restrict__ mean, const float* __restrict__ var, int N, int Np, int C, int Cp, int kh, int kw, int Kp,
                                                  bf16* __restrict__ wp, float* __restrict__ bias)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)Np * Kp) return;
    const int k = (int)(i % Kp), n = (int)(i / Kp);
    float v = 0.f, s = 0.f;
    if (n < N) {
        s = gamma[n] / sqrtf(var[n] + 1e-3f);
        if (k < kh * kw * Cp) {
            const int tap = k / Cp, c = k - tap * Cp, ky = tap / kw, kx = tap - ky * kw;
            if (c < C) v = w[(((int64_t)n * C + c) * kh + ky) * kw + kx] * s;
        }
    }
    const bf16 hi = (bf16)v;
    wp[(int64_t)n * 2 * Kp + k] = hi;
    wp[(int64_t)n * 2 * Kp + Kp + k] = (bf16)(v - (float)hi);
    if (k == 0) bias[n] = n < N ? beta[n] - mean[n] * s : 0.f;
}

// Plan 2 (half precision, ONE filter term): one block per packed filter row.  W'[n][k] as k_inc_pack folds it, divided by the row's power-of-two scale
// 2^(floor(log2 max|W'[n]|) + 1) -- the largest element lands in [0.5, 1) exactly -- and rounded to half; deq[n] = that scale (1 for an all-zero / pad row).
__global__ __launch_bounds__(256) void k_inc_pack_f16(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ mean, const float* __restrict__ var, int N, int C, int Cp, int kh, int kw, int Kp,
                                                      _Float16* __restrict__ wp, float* __restrict__ bias, float* __restrict__ deq)
{
    __shared__ float s_max[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float s = n < N ? gamma[n] / sqrtf(var[n] + 1e-3f) : 0.f;
    auto folded = [&](int k) {
        if (n >= N || k >= kh * kw * Cp) return 0.f;
        const int tap = k / Cp, c = k - tap * Cp, ky = tap / kw, kx = tap - ky * kw;
        return c < C ? w[(((int64_t)n * C + c) * kh + ky) * kw + kx] * s : 0.f;
    };
    float mx = 0.f;
    for (int k = tid; k < Kp; k += 256) mx = fmaxf(mx, fabsf(folded(k)));
    s_max[tid] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) { if (tid < h) s_max[tid] = fmaxf(s_max[tid], s_max[tid + h]); __syncthreads(); }
    mx = s_max[0];
    float scale = 1.0f;
    if (mx > 0.f) { int e; (void)frexpf(mx, &e); scale = ldexpf(1.0f, e); }         // mx = m * 2^e, m in [0.5, 1)
    const float inv = 1.0f / scale;                                                  // (a power of two: exact)
    for (int k = tid; k < Kp; k += 256) wp[(int64_t)n * Kp + k] = (_Float16)(folded(k) * inv);
    if (tid == 0) { bias[n] = n < N ? beta[n] - mean[n] * s : 0.f; deq[n] = scale; }
}

// The stem's and the pools' launches, as the plan (IncBuilder) and the debug entry points (natinf_debug_inc_stem / natinf_debug_inc_pool) both make them.
// stem: blockIdx.y = (sample, output row), threads over (output column, 4-column slot of a patch row of row_width = 64 | 32 columns)
inline void launch_inc_stem(const void* img, int is_u8, int H, int W, unsigned short* out, int B, int f16, int row_width, hipStream_t s) {
    hipLaunchKernelGGL(k_inc_stem, dim3((unsigned)((149 * (row_width / 4) + 255) / 256), (unsigned)(B * 149)), dim3(256), 0, s, img, is_u8, H, W, out, B, f16,
                       row_width == 64 ? 4 : 3);
}
// pool: one thread per (sample, output row, 8-channel chunk); the caller has checked that their number fits `unsigned`
inline void launch_inc_pool(bool f16, int mode, int stride, int pad, int B, int H, int W, int C, const unsigned short* x, int x_ld, unsigned short* out, int out_ld,
                            hipStream_t s) {
    const int Ho = (H + 2 * pad - 3) / stride + 1, Wo = (W + 2 * pad - 3) / stride + 1;
    const unsigned total = (unsigned)((int64_t)B * Ho * (C / 8));
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)(((uint64_t)total + 255) / 256)), dim3(256), 0, s, x, H, W, x_ld, C, pad, Ho, Wo, out, out_ld, total);
    };
    const int sel = (f16 ? 4 : 0) + (mode ? 2 : 0) + (stride == 2 ? 1 : 0);
    switch (sel) {
        case 0: go(&k_inc_pool<0, 0, 1>); break;  case 1: go(&k_inc_pool<0, 0, 2>); break;  case 2: go(&k_inc_pool<0, 1, 1>); break;  case 3: go(&k_inc_pool<0, 1, 2>); break;
        case 4: go(&k_inc_pool<1, 0, 1>); break;  case 5: go(&k_inc_pool<1, 0, 2>); break;  case 6: go(&k_inc_pool<1, 1, 1>); break;  default: go(&k_inc_pool<1, 1, 2>); break;
    }
}

}  // namespace ncsn

struct natinf_inception : EngineCore {
    int H = 0, W = 0;
    int input_u8 = 1;                    // per-forward
    int conv_mode = 1;                   // g_inc_conv when the plan was built
};
int g_inc_conv = 2;                      // natinf_set_inception_conv: 2 = k_conv_ring on half-precision activations and ONE half-precision filter term, 1 = k_conv_ring on bf16 with
                                         // the two-term filters, 0 = k_inc_im2col + GEMM (the round-3 / 4 plan)

int g_inc_tile192 = 1;                   // (NATINF_INC_TILE192=0 in the environment: A/B runs without the 128 x 192 tile)
template <class Cfg, class K>
inline void launch_conv_ring(K kernel, const GemmArgs& g, const ncsn::ConvGeom& cv, hipStream_t s) {
    const int nM = (g.M + Cfg::BM_ - 1) / Cfg::BM_, nN = (g.N + Cfg::BN_ - 1) / Cfg::BN_;
    hipLaunchKernelGGL(kernel, dim3(nM * nN), dim3(Cfg::THREADS), Cfg::LDS_BYTES, s, g, cv);
}
using CfgC256x128 = ncsn::RingCfg<2, 2, 8, 4, 3>; using CfgC256x64 = ncsn::RingCfg<4, 1, 4, 4, 3>; using CfgC128x128 = ncsn::RingCfg<2, 2, 4, 4, 4>;
using CfgC128x192 = ncsn::RingCfg<2, 2, 4, 6, 3>;          // N in (128, 192]: the 17 x 17 blocks' 160 / 192-channel convolutions (two 128-wide column tiles wasted a quarter of the matrix work)
bool configure_conv_ring() {
    return set_lds<CfgC256x128>(&ncsn::k_conv_ring<2, 2, 8, 4, 3>) && set_lds<CfgC256x64>(&ncsn::k_conv_ring<4, 1, 4, 4, 3>) &&
           set_lds<CfgC128x128>(&ncsn::k_conv_ring<2, 2, 4, 4, 4>) &&
           set_lds<CfgC256x128>(&ncsn::k_conv_ring<2, 2, 8, 4, 3, true>) && set_lds<CfgC256x64>(&ncsn::k_conv_ring<4, 1, 4, 4, 3, true>) &&
           set_lds<CfgC128x128>(&ncsn::k_conv_ring<2, 2, 4, 4, 4, true>) && set_lds<CfgC128x192>(&ncsn::k_conv_ring<2, 2, 4, 6, 3, true>);
}

namespace {

struct IncBuilder : PlanBuilder {
    natinf_inception& E;
    explicit IncBuilder(natinf_inception& e) : PlanBuilder(e), E(e) {}

    struct Ten { int64_t off = -1; int H = 0, W = 0, C = 0, ld = 0, coff = 0; };
    const bool implicit = g_inc_conv != 0, f16 = g_inc_conv == 2;
    int64_t zero_page = -1;
    // (implicit plan: a fresh tensor's row stride is its channel count padded to 32 -- the pad channels are written as zeros by the producing convolution)
    int cpad(int C) const { return implicit ? (int)align_up(C, 32) : C; }
    Ten new_ten(int H, int W, int C) { Ten t; t.ld = cpad(C); t.off = arena.alloc((int64_t)H * W * t.ld * 2); t.H = H; t.W = W; t.C = C; return t; }
    static Ten slice(const Ten& t, int coff, int C) { Ten s = t; s.coff = t.coff + coff; s.C = C; return s; }
    static bf16* ptr_of(const Ctx& c, const Ten& t) { return c.at<bf16>(t.off) + t.coff; }

    struct PackedConv { int64_t w, b; int Kp; int64_t deq = -1; };
    // cin_p / cout_p: channels per tap of the packed K order / packed filter rows (== cin / cout in the im2col plan and for the stem)
    PackedConv take_conv(int cin, int cout, int kh, int kw, int cin_p = 0, int cout_p = 0, int kalign = 0) {
        if (!cin_p) cin_p = cin;
        if (!cout_p) cout_p = cout;
        if (!kalign) kalign = implicit && cin_p % 32 == 0 ? 32 : 64;                                                  // (the im2col plan's GEMMs: 64-wide K-tiles)
        const int K = kh * kw * cin, Kp = (int)align_up(kh * kw * cin_p, kalign);
        const int64_t pw = take((int64_t)cout * K), pg = take(cout), pb = take(cout), pm = take(cout), pv = take(cout);
        if (f16) {                                                    // one half-precision term + the rows' power-of-two scales
            PackedConv r{wres((int64_t)cout_p * Kp * 2), wres((int64_t)cout_p * 4), Kp, wres((int64_t)cout_p * 4)};
            E.packs.push_back([=](const PackCtx& p) {
                hipLaunchKernelGGL(k_inc_pack_f16, dim3(cout_p), dim3(256), 0, p.stream, p.params + pw, p.params + pg, p.params + pb, p.params + pm, p.params + pv,
                                   cout, cin, cin_p, kh, kw, Kp, reinterpret_cast<_Float16*>(p.packed + r.w), reinterpret_cast<float*>(p.packed + r.b),
                                   reinterpret_cast<float*>(p.packed + r.deq));
            });
            return r;
        }
        PackedConv r{wres((int64_t)cout_p * 2 * Kp * 2), wres((int64_t)cout_p * 4), Kp};
        E.packs.push_back([=](const PackCtx& p) {
            hipLaunchKernelGGL(k_inc_pack, dim3(grid1d((int64_t)cout_p * Kp, 256, 1 << 30)), dim3(256), 0, p.stream, p.params + pw, p.params + pg, p.params + pb,
                               p.params + pm, p.params + pv, cout, cout_p, cin, cin_p, kh, kw, Kp, reinterpret_cast<bf16*>(p.packed + r.w),
                               reinterpret_cast<float*>(p.packed + r.b));
        });
        return r;
    }
    static void gemm_relu(const Ctx& c, const bf16* a, int a_ld, int K, int64_t M, const PackedConv& pc, int N, bf16* dst, int dst_ld) {
        GemmArgs g = gemm_defaults();
        g.a0 = a; g.a0_ld = a_ld; g.a0_C = K; g.M = (int)M; g.N = N;
        g.a1 = a; g.a1_ld = a_ld; g.a1_C = K;                        // second K segment: the same operand against the filters' residual term
        g.b = c.w<bf16>(pc.w); g.b_ld = 2 * pc.Kp; g.bias_n = c.w<float>(pc.b); g.act = ACT_RELU;
        g.c = dst; g.c_ld = dst_ld; g.log_rows_per_sample = 30;
        launch_gemm(g, c.stream);
    }
    // BasicConv2d x -> dst (a fresh tensor, or a channel slice of a concat buffer)
    // one k_conv_ring launch: relu(conv(x) + bias) into y (bias / filters of pc; h: half-precision plan -- one filter term, column scales)
    static void launch_conv(const Ctx& c, const bf16* x, int x_ld, int H, int W, int Ho, int Wo, int kh, int kw, int stride, int ph, int pw, int cin_p, int cout_p,
                            const PackedConv& pc, bf16* y, int y_ld, int64_t zero_page, bool h) {
        GemmArgs g = gemm_defaults();
        g.a0 = x; g.a0_ld = x_ld; g.a0_C = cin_p; g.M = c.B * Ho * Wo; g.N = cout_p;
        g.b = c.w<bf16>(pc.w); g.b_ld = (h ? 1 : 2) * pc.Kp; g.bias_n = c.w<float>(pc.b); g.act = ACT_RELU;
        if (h) g.deq_n = c.w<float>(pc.deq);
        g.c = y; g.c_ld = y_ld; g.log_rows_per_sample = 30;
        ncsn::ConvGeom cv{H, W, Ho, Wo, kh, kw, stride, ph, pw, cin_p / 32, h ? 1 : 2, c.w<char>(zero_page)};
        const int64_t t256 = ((int64_t)g.M + 255) / 256;
        const int shape = cout_p <= 64 ? 0 : (t256 * ((cout_p + 127) / 128) >= 2 * NUM_CU ? 1 : 2);
        if (h) {
            if (cout_p > 128 && cout_p <= 192 && g_inc_tile192) launch_conv_ring<CfgC128x192>(&ncsn::k_conv_ring<2, 2, 4, 6, 3, true>, g, cv, c.stream);
            else if (shape == 0) launch_conv_ring<CfgC256x64>(&ncsn::k_conv_ring<4, 1, 4, 4, 3, true>, g, cv, c.stream);
            else if (shape == 1) launch_conv_ring<CfgC256x128>(&ncsn::k_conv_ring<2, 2, 8, 4, 3, true>, g, cv, c.stream);
            else launch_conv_ring<CfgC128x128>(&ncsn::k_conv_ring<2, 2, 4, 4, 4, true>, g, cv, c.stream);
        } else {
            if (shape == 0) launch_conv_ring<CfgC256x64>(&ncsn::k_conv_ring<4, 1, 4, 4, 3>, g, cv, c.stream);
            else if (shape == 1) launch_conv_ring<CfgC256x128>(&ncsn::k_conv_ring<2, 2, 8, 4, 3>, g, cv, c.stream);
            else launch_conv_ring<CfgC128x128>(&ncsn::k_conv_ring<2, 2, 4, 4, 4>, g, cv, c.stream);
        }
    }
    Ten conv(const Ten& x, int cout, int kh, int kw, int stride, int ph, int pw, const Ten* into = nullptr) {
        const int Ho = (x.H + 2 * ph - kh) / stride + 1, Wo = (x.W + 2 * pw - kw) / stride + 1;
        if (implicit) {
            // the implicit GEMM: K-tiles of one tap x 32 channels straight from x; a fresh output tensor gets its pad channels (zero filter rows) written too
            const int cin_p = (int)align_up(x.C, 32);
            const int cout_p = into ? cout : (int)align_up(cout, 32);
            const PackedConv pc = take_conv(x.C, cout, kh, kw, cin_p, cout_p);
            Ten y = into ? *into : new_ten(Ho, Wo, cout);
            const Ten xin = x;
            const int64_t zp = zero_page;
            const bool h = f16;
            op([=](const Ctx& c) { launch_conv(c, ptr_of(c, xin), xin.ld, xin.H, xin.W, Ho, Wo, kh, kw, stride, ph, pw, cin_p, cout_p, pc, ptr_of(c, y), y.ld, zp, h); });
            return y;
        }
        const PackedConv pc = take_conv(x.C, cout, kh, kw);
        Ten y = into ? *into : new_ten(Ho, Wo, cout);
        const bool direct = kh == 1 && kw == 1 && stride == 1 && x.C % 64 == 0 && x.coff % 8 == 0;
        const int64_t col = direct ? -1 : arena.alloc((int64_t)Ho * Wo * pc.Kp * 2);
        const Ten xin = x;
        op([=](const Ctx& c) {
            const int64_t M = (int64_t)c.B * Ho * Wo;
            if (direct) { gemm_relu(c, ptr_of(c, xin), xin.ld, xin.C, M, pc, cout, ptr_of(c, y), y.ld); return; }
            const int64_t total = M * (pc.Kp / 8);
            hipLaunchKernelGGL(k_inc_im2col, dim3(grid1d(total, 256, 1 << 30)), dim3(256), 0, c.stream, ptr_of(c, xin), xin.H, xin.W, xin.ld, xin.C, kh, kw, stride,
                               ph, pw, Ho, Wo, pc.Kp, c.at<bf16>(col), total);
            gemm_relu(c, c.at<bf16>(col), pc.Kp, pc.Kp, M, pc, cout, ptr_of(c, y), y.ld);
        });
        if (col >= 0) arena.release(col);
        return y;
    }
    Ten pool(const Ten& x, int stride, int pad, int mode, const Ten* into = nullptr) {
        const int Ho = (x.H + 2 * pad - 3) / stride + 1, Wo = (x.W + 2 * pad - 3) / stride + 1;
        Ten y = into ? *into : new_ten(Ho, Wo, x.C);
        const Ten xin = x;
        const bool h = f16;
        op([=](const Ctx& c) {
            launch_inc_pool(h, mode, stride, pad, c.B, xin.H, xin.W, xin.C, reinterpret_cast<const unsigned short*>(ptr_of(c, xin)), xin.ld,
                            reinterpret_cast<unsigned short*>(ptr_of(c, y)), y.ld, c.stream);
        });
        return y;
    }
    void free_ten(Ten& t) { arena.release(t.off); t.off = -1; }

    Ten inception_a(Ten x, int pf) {
        Ten out = new_ten(x.H, x.W, 64 + 64 + 96 + pf);
        Ten s0 = slice(out, 0, 64), s1 = slice(out, 64, 64), s2 = slice(out, 128, 96), s3 = slice(out, 224, pf);
        conv(x, 64, 1, 1, 1, 0, 0, &s0);
        Ten t = conv(x, 48, 1, 1, 1, 0, 0); conv(t, 64, 5, 5, 1, 2, 2, &s1); free_ten(t);
        t = conv(x, 64, 1, 1, 1, 0, 0); Ten u = conv(t, 96, 3, 3, 1, 1, 1); free_ten(t); conv(u, 96, 3, 3, 1, 1, 1, &s2); free_ten(u);
        t = pool(x, 1, 1, 1); conv(t, pf, 1, 1, 1, 0, 0, &s3); free_ten(t);
        free_ten(x);
        return out;
    }
    Ten inception_b(Ten x) {
        const int Ho = (x.H - 3) / 2 + 1;
        Ten out = new_ten(Ho, Ho, 384 + 96 + x.C);
        Ten s0 = slice(out, 0, 384), s1 = slice(out, 384, 96), s2 = slice(out, 480, x.C);
        conv(x, 384, 3, 3, 2, 0, 0, &s0);
        Ten t = conv(x, 64, 1, 1, 1, 0, 0); Ten u = conv(t, 96, 3, 3, 1, 1, 1); free_ten(t); conv(u, 96, 3, 3, 2, 0, 0, &s1); free_ten(u);
        pool(x, 2, 0, 0, &s2);
        free_ten(x);
        return out;
    }
    Ten inception_c(Ten x, int c7) {
        Ten out = new_ten(x.H, x.W, 768);
        Ten s0 = slice(out, 0, 192), s1 = slice(out, 192, 192), s2 = slice(out, 384, 192), s3 = slice(out, 576, 192);
        conv(x, 192, 1, 1, 1, 0, 0, &s0);
        Ten t = conv(x, c7, 1, 1, 1, 0, 0); Ten u = conv(t, c7, 1, 7, 1, 0, 3); free_ten(t); conv(u, 192, 7, 1, 1, 3, 0, &s1); free_ten(u);
        t = conv(x, c7, 1, 1, 1, 0, 0);
        u = conv(t, c7, 7, 1, 1, 3, 0); free_ten(t);
        t = conv(u, c7, 1, 7, 1, 0, 3); free_ten(u);
        u = conv(t, c7, 7, 1, 1, 3, 0); free_ten(t);
        conv(u, 192, 1, 7, 1, 0, 3, &s2); free_ten(u);
        t = pool(x, 1, 1, 1); conv(t, 192, 1, 1, 1, 0, 0, &s3); free_ten(t);
        free_ten(x);
        return out;
    }
    Ten inception_d(Ten x) {
        const int Ho = (x.H - 3) / 2 + 1;
        Ten out = new_ten(Ho, Ho, 320 + 192 + x.C);
        Ten s0 = slice(out, 0, 320), s1 = slice(out, 320, 192), s2 = slice(out, 512, x.C);
        Ten t = conv(x, 192, 1, 1, 1, 0, 0); conv(t, 320, 3, 3, 2, 0, 0, &s0); free_ten(t);
        t = conv(x, 192, 1, 1, 1, 0, 0);
        Ten u = conv(t, 192, 1, 7, 1, 0, 3); free_ten(t);
        t = conv(u, 192, 7, 1, 1, 3, 0); free_ten(u);
        conv(t, 192, 3, 3, 2, 0, 0, &s1); free_ten(t);
        pool(x, 2, 0, 0, &s2);
        free_ten(x);
        return out;
    }
    Ten inception_e(Ten x, int pool_mode) {                 // pool_mode 1: FIDInceptionE_1 (average, valid count), 0: FIDInceptionE_2 (max)
        Ten out = new_ten(x.H, x.W, 2048);
        Ten s0 = slice(out, 0, 320), s1a = slice(out, 320, 384), s1b = slice(out, 704, 384), s2a = slice(out, 1088, 384), s2b = slice(out, 1472, 384),
            s3 = slice(out, 1856, 192);
        conv(x, 320, 1, 1, 1, 0, 0, &s0);
        Ten t = conv(x, 384, 1, 1, 1, 0, 0); conv(t, 384, 1, 3, 1, 0, 1, &s1a); conv(t, 384, 3, 1, 1, 1, 0, &s1b); free_ten(t);
        t = conv(x, 448, 1, 1, 1, 0, 0); Ten u = conv(t, 384, 3, 3, 1, 1, 1); free_ten(t);
        conv(u, 384, 1, 3, 1, 0, 1, &s2a); conv(u, 384, 3, 1, 1, 1, 0, &s2b); free_ten(u);
        t = pool(x, 1, 1, pool_mode); conv(t, 192, 1, 1, 1, 0, 0, &s3); free_ten(t);
        free_ten(x);
        return out;
    }

    void build() {
        const int H = E.H, W = E.W;
        E.conv_mode = g_inc_conv;
        if (implicit) {                                               // the page of zeros padding taps are fetched from
            zero_page = wres(256);
            const int64_t zp = zero_page;
            E.packs.push_back([=](const PackCtx& p) { (void)hipMemsetAsync(p.packed + zp, 0, 256, p.stream); });
        }
        // ---- stem: resize + normalise + im2col of Conv2d_1a_3x3 (3 -> 32, stride 2), then the GEMM
        const int kr = f16 ? 32 : 64;                                // K = 27 padded to the patch rows' width: 64 for the GEMM of plans 0 / 1, 32 on k_conv_ring
        const PackedConv p1a = take_conv(3, 32, 3, 3, 0, 0, kr);
        Ten x = new_ten(149, 149, 32);
        {
            const int64_t col = arena.alloc((int64_t)149 * 149 * kr * 2);
            const Ten y = x;
            natinf_inception* eng = &E;
            const bool h = f16;
            const int64_t zp = zero_page;
            op([=](const Ctx& c) {
                const int64_t M = (int64_t)c.B * 149 * 149;
                launch_inc_stem(reinterpret_cast<const void*>(c.x), eng->input_u8, H, W, c.at<unsigned short>(col), c.B, (int)h, kr, c.stream);
                // half-precision plan: the GEMM over the patch rows as a 1x1 "convolution" of k_conv_ring (32 channels per row: one K-tile, 256 x 64 tiles)
                if (h) launch_conv(c, c.at<bf16>(col), kr, 149, 149, 149, 149, 1, 1, 1, 0, 0, kr, 32, p1a, ptr_of(c, y), y.ld, zp, true);
                else gemm_relu(c, c.at<bf16>(col), 64, 64, M, p1a, 32, ptr_of(c, y), y.ld);
            });
            arena.release(col);
        }
        Ten t = conv(x, 32, 3, 3, 1, 0, 0); free_ten(x);             // Conv2d_2a_3x3: 147
        x = conv(t, 64, 3, 3, 1, 1, 1); free_ten(t);                 // Conv2d_2b_3x3
        t = pool(x, 2, 0, 0); free_ten(x);                           // 73
        x = conv(t, 80, 1, 1, 1, 0, 0); free_ten(t);                 // Conv2d_3b_1x1
        t = conv(x, 192, 3, 3, 1, 0, 0); free_ten(x);                // Conv2d_4a_3x3: 71
        x = pool(t, 2, 0, 0); free_ten(t);                           // 35
        x = inception_a(x, 32); x = inception_a(x, 64); x = inception_a(x, 64);          // Mixed_5b, 5c, 5d
        x = inception_b(x);                                                              // Mixed_6a: 17
        x = inception_c(x, 128); x = inception_c(x, 160); x = inception_c(x, 160); x = inception_c(x, 192);      // Mixed_6b .. 6e
        x = inception_d(x);                                                              // Mixed_7a: 8
        x = inception_e(x, 1); x = inception_e(x, 0);                                    // Mixed_7b, 7c
        const Ten last = x;
        const bool h = f16;
        op([=](const Ctx& c) {
            const int64_t total = (int64_t)c.B * 2048;
            hipLaunchKernelGGL(k_inc_global_avg, dim3(grid1d(total, 256, 1 << 30)), dim3(256), 0, c.stream, reinterpret_cast<const unsigned short*>(ptr_of(c, last)),
                               last.H * last.W, 2048, c.out, total, (int)h);
        });
        finish();
    }
};

}  // namespace

extern "C" {

int natinf_inception_create(natinf_inception_t* out, int in_h, int in_w) {
    if (!out || in_h <= 0 || in_w <= 0 || in_h > 4096 || in_w > 4096) return NATINF_EINVAL;
    natinf_inception* e = new natinf_inception();
    e->H = in_h; e->W = in_w;
    if (const char* t = getenv("NATINF_INC_TILE192")) g_inc_tile192 = atoi(t) != 0;
    IncBuilder b(*e);
    b.build();
    *out = e;
    return NATINF_OK;
}
int natinf_inception_destroy(natinf_inception_t h) { if (!h) return NATINF_EINVAL; delete h; return NATINF_OK; }
// k_conv_ring on caller-supplied operands (tests): see include/natinf_inception.h
int natinf_debug_conv_ring(int tile, int f16, int B, int H, int W, int cin_p, int x_ld, int cout, int kh, int kw, int stride, int ph, int pw, int passes,
                           const void* x, const void* w_packed, const float* bias, const float* col_scale, const void* zeros, void* out, int out_ld,
                           natinf_stream_t stream) {
    if (!x || !w_packed || !zeros || !out || B <= 0 || H <= 0 || W <= 0 || cin_p <= 0 || cin_p % 32 || x_ld < cin_p || x_ld % 8 || cout <= 0 || cout % 8 || out_ld < cout ||
        out_ld % 8 || kh <= 0 || kw <= 0 || stride <= 0 || ph < 0 || pw < 0 || (passes != 1 && passes != 2) || tile < 0 || tile > 3 || (tile == 3 && !f16)) return NATINF_EINVAL;
    const int Ho = (H + 2 * ph - kh) / stride + 1, Wo = (W + 2 * pw - kw) / stride + 1;
    if (Ho <= 0 || Wo <= 0 || (int64_t)B * Ho * Wo >= (1LL << 31)) return NATINF_EINVAL;
    static bool configured = false;
    if (!configured) { if (!configure_gemm_kernels()) return NATINF_ENODEV; configured = true; }
    GemmArgs g = gemm_defaults();
    g.a0 = (const bf16*)x; g.a0_ld = x_ld; g.a0_C = cin_p; g.M = B * Ho * Wo; g.N = cout;
    g.b = (const bf16*)w_packed; g.b_ld = passes * kh * kw * cin_p; g.bias_n = bias; g.deq_n = col_scale; g.act = ACT_RELU;
    g.c = out; g.c_ld = out_ld; g.log_rows_per_sample = 30;
    ncsn::ConvGeom cv{H, W, Ho, Wo, kh, kw, stride, ph, pw, cin_p / 32, passes, zeros};
    hipStream_t s = (hipStream_t)stream;
    if (f16) {
        if (tile == 0) launch_conv_ring<CfgC256x64>(&ncsn::k_conv_ring<4, 1, 4, 4, 3, true>, g, cv, s);
        else if (tile == 1) launch_conv_ring<CfgC256x128>(&ncsn::k_conv_ring<2, 2, 8, 4, 3, true>, g, cv, s);
        else if (tile == 2) launch_conv_ring<CfgC128x128>(&ncsn::k_conv_ring<2, 2, 4, 4, 4, true>, g, cv, s);
        else launch_conv_ring<CfgC128x192>(&ncsn::k_conv_ring<2, 2, 4, 6, 3, true>, g, cv, s);
    } else {
        if (tile == 0) launch_conv_ring<CfgC256x64>(&ncsn::k_conv_ring<4, 1, 4, 4, 3>, g, cv, s);
        else if (tile == 1) launch_conv_ring<CfgC256x128>(&ncsn::k_conv_ring<2, 2, 8, 4, 3>, g, cv, s);
        else launch_conv_ring<CfgC128x128>(&ncsn::k_conv_ring<2, 2, 4, 4, 4>, g, cv, s);
    }
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
// the engine's other kernels on caller-supplied operands (tests): contracts in include/natinf_inception.h
static inline bool inc_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int natinf_debug_inc_stem(const void* images, int input_kind, int B, int H, int W, int f16, int row_width, void* out, natinf_stream_t stream) {
    if (!images || !out || ((uintptr_t)out & 7) || (input_kind != NATINF_INCEPTION_U8_HWC && input_kind != NATINF_INCEPTION_F32_CHW) || B <= 0 || H <= 0 || W <= 0 ||
        H > 4096 || W > 4096 || (f16 != 0 && f16 != 1) || (row_width != 32 && row_width != 64) || (int64_t)B * 149 * 149 >= (1LL << 31)) return NATINF_EINVAL;
    if (input_kind == NATINF_INCEPTION_F32_CHW && ((uintptr_t)images & 3)) return NATINF_EINVAL;
    ncsn::launch_inc_stem(images, input_kind == NATINF_INCEPTION_U8_HWC, H, W, (unsigned short*)out, B, f16, row_width, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_debug_inc_pool(int f16, int mode, int stride, int pad, int B, int H, int W, int C, const void* x, int x_ld, void* out, int out_ld,
                          natinf_stream_t stream) {
    if (!x || !out || !inc_al16(x) || !inc_al16(out) || (f16 != 0 && f16 != 1) || (mode != 0 && mode != 1) || (stride != 1 && stride != 2) || (pad != 0 && pad != 1) ||
        B <= 0 || H <= 0 || W <= 0 || H > 65536 || W > 65536 || H + 2 * pad < 3 || W + 2 * pad < 3 || C < 8 || C % 8 || x_ld < C || x_ld % 8 || out_ld < C || out_ld % 8) return NATINF_EINVAL;
    const int Ho = (H + 2 * pad - 3) / stride + 1;
    if ((int64_t)B * Ho * (C / 8) >= (1LL << 32)) return NATINF_EINVAL;
    ncsn::launch_inc_pool(f16 != 0, mode, stride, pad, B, H, W, C, (const unsigned short*)x, x_ld, (unsigned short*)out, out_ld, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_debug_inc_global_avg(int f16, int B, int HW, int C, const void* x, float* out, natinf_stream_t stream) {
    if (!x || !out || ((uintptr_t)x & 1) || ((uintptr_t)out & 3) || (f16 != 0 && f16 != 1) || B <= 0 || HW <= 0 || C <= 0 || (int64_t)B * C >= (1LL << 31))
        return NATINF_EINVAL;
    const int64_t total = (int64_t)B * C;
    hipLaunchKernelGGL(ncsn::k_inc_global_avg, dim3(grid1d(total, 256, 1 << 30)), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, HW, C, out, total, f16);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_debug_inc_pack(int f16, const float* w, const float* gamma, const float* beta, const float* mean, const float* var, int N, int Np, int C, int Cp,
                          int kh, int kw, int Kp, void* wp, float* bias, float* deq, natinf_stream_t stream) {
    if (!w || !gamma || !beta || !mean || !var || !wp || !bias || (f16 != 0 && f16 != 1) || (f16 && !deq) || N <= 0 || Np < N || C <= 0 || Cp < C || kh <= 0 || kw <= 0 ||
        Kp <= 0 || Kp % 32 || (int64_t)kh * kw * Cp > Kp || (int64_t)Np * 2 * Kp >= (1LL << 31)) return NATINF_EINVAL;
    if (((uintptr_t)w | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)mean | (uintptr_t)var | (uintptr_t)bias | (uintptr_t)deq) & 3 || ((uintptr_t)wp & 1))
        return NATINF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (f16) hipLaunchKernelGGL(ncsn::k_inc_pack_f16, dim3(Np), dim3(256), 0, s, w, gamma, beta, mean, var, N, C, Cp, kh, kw, Kp, (_Float16*)wp, bias, deq);
    else hipLaunchKernelGGL(ncsn::k_inc_pack, dim3(grid1d((int64_t)Np * Kp, 256, 1 << 30)), dim3(256), 0, s, w, gamma, beta, mean, var, N, Np, C, Cp, kh, kw, Kp, (bf16*)wp,
                            bias);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_debug_inc_im2col(int B, int H, int W, int ld, int C, int kh, int kw, int stride, int ph, int pw, int Kp, const void* x, void* out,
                            natinf_stream_t stream) {
    if (!x || !out || !inc_al16(x) || !inc_al16(out) || B <= 0 || H <= 0 || W <= 0 || H > 65536 || W > 65536 || kh <= 0 || kw <= 0 || stride <= 0 || ph < 0 || pw < 0 || C < 8 || C % 8 ||
        ld < C || ld % 8 || Kp <= 0 || Kp % 8 || (int64_t)kh * kw * C > Kp || (int64_t)H + 2 * (int64_t)ph < kh || (int64_t)W + 2 * (int64_t)pw < kw ||
        ph > 4096 || pw > 4096) return NATINF_EINVAL;
    const int Ho = (H + 2 * ph - kh) / stride + 1, Wo = (W + 2 * pw - kw) / stride + 1;
    if ((double)B * Ho * Wo * (Kp / 8) >= 2147483648.0) return NATINF_EINVAL;
    const int64_t total = (int64_t)B * Ho * Wo * (Kp / 8);
    hipLaunchKernelGGL(ncsn::k_inc_im2col, dim3(grid1d(total, 256, 1 << 30)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, H, W, ld, C, kh, kw, stride, ph, pw,
                       Ho, Wo, Kp, (bf16*)out, total);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
int natinf_set_inception_conv(int mode) { if (mode < 0 || mode > 2) return NATINF_EINVAL; g_inc_conv = mode; return NATINF_OK; }
int64_t natinf_inception_param_count(natinf_inception_t h) { return h ? h->n_params : NATINF_EINVAL; }
int64_t natinf_inception_packed_bytes(natinf_inception_t h) { return h ? h->packed_bytes : NATINF_EINVAL; }
int64_t natinf_inception_workspace_bytes(natinf_inception_t h, int max_batch) { return h && max_batch > 0 ? h->ws_per_image * (int64_t)max_batch : NATINF_EINVAL; }
int natinf_inception_load(natinf_inception_t h, const float* params_f32, int64_t n_params, void* packed, int64_t packed_bytes, natinf_stream_t stream) {
    return h ? h->load(params_f32, n_params, packed, packed_bytes, (hipStream_t)stream) : NATINF_EINVAL;
}
int natinf_inception_forward(natinf_inception_t h, const void* images, int input_kind, float* features, int B, void* workspace, int64_t workspace_bytes,
                             natinf_stream_t stream) {
    if (!h || !images || (input_kind != NATINF_INCEPTION_U8_HWC && input_kind != NATINF_INCEPTION_F32_CHW)) return NATINF_EINVAL;
    if ((int64_t)B * 149 * 149 >= (1LL << 31)) return NATINF_EINVAL;
    h->input_u8 = input_kind == NATINF_INCEPTION_U8_HWC;
    const float* x = reinterpret_cast<const float*>(images);
    return h->run(x, x, features, B, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
