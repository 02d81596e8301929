// fit.hip -- the fp64 Gram matrix of the coefficient fitter (include/natinf_fit.h): per image a 32 x 32 x E product of the
// stacked vectors with their own transpose on v_mfma_f64_16x16x4_f64, upper tiles only, the history streamed once in 16-byte accesses.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "natinf.h"
#include "natinf_fit.h"

namespace fit {

constexpr int WAVES = NATINF_FIT_WAVES, THREADS = WAVES * 64;
constexpr int STEP = 16;                   // elements per wave step: four lanes quarters q x four elements, one 16 x 16 x 4 issue per element of a quarter
constexpr int LD = 32;                     // row length of the assembled matrix

typedef double d4 __attribute__((ext_vector_type(4)));

struct Args {
    const double* hist;
    const float* noise;
    const float* target;
    double* gram;
    int64_t stride, epi;
    int n_rows;
    int32_t rows[NATINF_FIT_MAX_ROWS];
};

// One vector of the stack as a lane reads it.  Every lane issues the same two 16-byte loads and no branch depends on what kind of row it holds, so the
// loads of several steps are in flight together: an fp64 row gives the values e .. e + 3 in a and b; an fp32 row gives them in a
// (b repeats a's address: nothing past the row's last 16 bytes is touched); a pad row of a tile reads the image's noise and is masked to zero, as is a
// read at or past epi, which is made at element 0 instead.
struct Src {
    const char* base;
    uint32_t shift, off2;      // log2 of the element size; byte offset of the second load
    uint32_t f32, keep;        // all-ones masks: the row is fp32; the row is one of the M vectors
};
struct Raw { uint4 a, b; };

__device__ __forceinline__ Raw load_raw(const Src& v, int64_t e, int64_t epi)
{
    const char* p = v.base + ((e < epi ? e : (int64_t)0) << v.shift);
    return Raw{*(const uint4*)p, *(const uint4*)(p + v.off2)};
}

__device__ __forceinline__ double pick(float f, uint32_t lo, uint32_t hi, uint32_t f32, uint32_t keep)
{
    const double w = (double)f;
    const uint32_t wl = (uint32_t)__double2loint(w), wh = (uint32_t)__double2hiint(w);
    return __hiloint2double((int)(((wh & f32) | (hi & ~f32)) & keep), (int)(((wl & f32) | (lo & ~f32)) & keep));
}

__device__ __forceinline__ d4 widen4(const Raw& r, const Src& v, int64_t e, int64_t epi)
{
    const uint32_t keep = e < epi ? v.keep : 0u;
    d4 o;
    o[0] = pick(__uint_as_float(r.a.x), r.a.x, r.a.y, v.f32, keep);
    o[1] = pick(__uint_as_float(r.a.y), r.a.z, r.a.w, v.f32, keep);
    o[2] = pick(__uint_as_float(r.a.z), r.b.x, r.b.y, v.f32, keep);
    o[3] = pick(__uint_as_float(r.a.w), r.b.z, r.b.w, v.f32, keep);
    return o;
}

// NB: 16-row blocks of the stacked vectors (1: M <= 16, one tile; 2: the tiles (0,0), (0,1), (1,1)).
// A / B operand of the f64 16x16x4 form: lane l holds row (column) l & 15 at k = l >> 4; C / D: column l & 15, row (l >> 4) + 4 * reg.
// The sum over k is a sum over elements, so any assignment of elements to (issue, k) serves as long as A and B share it: lane quarter q = l >> 4
// reads elements 4 q .. 4 q + 3 of the step in 16-byte accesses, and issue j takes element 4 q + j of every quarter.
template <int NB>
__global__ __launch_bounds__(THREADS) void k_fit_gram(Args a)
{
    constexpr int NT = NB == 1 ? 1 : 3;
    __shared__ double part[WAVES][NT][256];
    __shared__ double full[(16 * NB) * LD];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 15, q = lane >> 4;
    const int64_t img = blockIdx.x, epi = a.epi;
    const int M = a.n_rows + 2;

    Src src[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int t = 16 * b + r;
        int32_t slot = 0;
#pragma unroll
        for (int u = 0; u < NATINF_FIT_MAX_ROWS; ++u) slot = (u == t) ? a.rows[u] : slot;      // static indices: the table stays in scalar registers
        const bool f64 = t < a.n_rows;
        const char* h = (const char*)(a.hist + (int64_t)slot * a.stride + img * epi);
        const char* f = (const char*)((t == a.n_rows + 1 ? a.target : a.noise) + img * epi);
        src[b] = Src{f64 ? h : f, f64 ? 3u : 2u, f64 ? 16u : 0u, f64 ? 0u : ~0u, t < M ? ~0u : 0u};
    }

    d4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};

    const int64_t n_steps = (epi + STEP - 1) / STEP;
    // two steps an iteration (a step past the last one is all zeros and leaves the sums as they are): the loads of both are issued before the first
    // issue waits for its operands
    for (int64_t s = wave; s < n_steps; s += 2 * WAVES) {
        Raw raw[2][NB];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int b = 0; b < NB; ++b) raw[h][b] = load_raw(src[b], (s + h * WAVES) * STEP + 4 * q, epi);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            d4 cur[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) cur[b] = widen4(raw[h][b], src[b], (s + h * WAVES) * STEP + 4 * q, epi);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[0][j], cur[0][j], acc[0], 0, 0, 0);
                if constexpr (NB == 2) {
                    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[0][j], cur[1][j], acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[1][j], cur[1][j], acc[2], 0, 0, 0);
                }
            }
        }
    }

#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) part[wave][t][(q + 4 * g) * 16 + r] = acc[t][g];
    __syncthreads();

    // the waves' sums in ascending wave order, into the assembled matrix: tile 0 = (0,0), 1 = (0,1), 2 = (1,1)
    for (int idx = threadIdx.x; idx < NT * 256; idx += THREADS) {
        const int t = idx >> 8, row = (idx >> 4) & 15, col = idx & 15;
        double sum = part[0][t][idx & 255];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) sum += part[w][t][idx & 255];
        full[(16 * (t >> 1) + row) * LD + 16 * ((t + 1) >> 1) + col] = sum;
    }
    __syncthreads();

    // both halves from the entry above the diagonal: the same bytes
    double* out = a.gram + img * (int64_t)(M * M);
    for (int idx = threadIdx.x; idx < M * M; idx += THREADS) {
        const int ra = idx / M, rb = idx - ra * M;
        out[idx] = full[min(ra, rb) * LD + max(ra, rb)];
    }
}

}  // namespace fit

extern "C" int natinf_fit_gram_f64(const double* hist, int64_t hist_stride, const int32_t* rows, int n_rows,
                                   const float* noise, const float* target,
                                   int64_t n_images, int64_t elems_per_image,
                                   double* gram, natinf_stream_t stream)
{
    const int64_t epi = elems_per_image;
    if (!hist || !rows || !noise || !target || !gram) return NATINF_EINVAL;
    if (n_rows < 1 || n_rows > NATINF_FIT_MAX_ROWS) return NATINF_EINVAL;
    if (epi < 4 || epi > ((int64_t)1 << 24) || epi % 4) return NATINF_EINVAL;
    if (n_images < 1 || n_images > ((int64_t)1 << 20)) return NATINF_EINVAL;
    if (hist_stride < n_images * epi || hist_stride % 2) return NATINF_EINVAL;
    if (((uintptr_t)hist | (uintptr_t)noise | (uintptr_t)target | (uintptr_t)gram) & 15) return NATINF_EINVAL;
    for (int t = 0; t < n_rows; ++t)
        if (rows[t] < 0 || (t && rows[t] <= rows[t - 1])) return NATINF_EINVAL;

    fit::Args a{};
    a.hist = hist; a.noise = noise; a.target = target; a.gram = gram;
    a.stride = hist_stride; a.epi = epi; a.n_rows = n_rows;
    for (int t = 0; t < n_rows; ++t) a.rows[t] = rows[t];
    hipStream_t s = (hipStream_t)stream;
    if (n_rows + 2 <= 16) hipLaunchKernelGGL(fit::k_fit_gram<1>, dim3((unsigned)n_images), dim3(fit::THREADS), 0, s, a);
    else                  hipLaunchKernelGGL(fit::k_fit_gram<2>, dim3((unsigned)n_images), dim3(fit::THREADS), 0, s, a);
    return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
}
