// prdc.hip -- the k-nearest-neighbour manifold metrics' kernels (prdc.h) and their C ABI (include/natinf_prdc.h); the nearest neighbours' indices
// (include/natinf_nn.h) and the kernel-distance row sums on the same sweep (include/natinf_kid.h), the Inception Score's row statistics on its logits (include/natinf_is.h) and the ideal denoiser, two sweeps around a row softmax
// (ideal.h; include/natinf_ideal.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "natinf.h"
#include "natinf_prdc.h"
#include "natinf_nn.h"
#include "natinf_kid.h"
#include "natinf_is.h"
#include "natinf_ideal.h"

namespace {
#include "prdc.h"
#include "ideal.h"

inline int launched() { return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH; }

constexpr int RESIDENT_BLOCKS = 512;     // 256 CUs x 2 blocks (46 KB of LDS, <= 256 VGPRs each)
constexpr int MAX_SPLITS = 64;
constexpr int MIN_SPLITS = 8;            // one column range per XCD: the blocks of a row block run beside each other and share its rows of A beyond the L2s

inline bool dims_ok(int d, int k) { return d >= 64 && d <= NATINF_PRDC_MAX_D && d % 64 == 0 && k >= 1 && k <= NATINF_PRDC_MAX_K; }
inline bool count_ok(int64_t n) { return n >= 1 && n <= NATINF_PRDC_MAX_N; }
inline bool self_ok(int64_t self_offset, int64_t n_rows, int64_t n_cols) { return self_offset >= -1 && (self_offset < 0 || self_offset + n_rows <= n_cols); }
inline bool aligned(const void* p, uintptr_t a) { return p && !((uintptr_t)p & (a - 1)); }

inline int64_t row_blocks(int64_t n_rows) { return (n_rows + prdc::BM - 1) / prdc::BM; }

// Blocks over the column tiles: as many as fill one round of resident blocks, eight at least.  A function of the shape only; the result does not depend
// on it (the k smallest of a set, an integer sum).
inline int splits_for(int64_t n_rows, int64_t n_cols) {
    const int64_t ctiles = (n_cols + prdc::BN - 1) / prdc::BN, smax = ctiles < MAX_SPLITS ? ctiles : MAX_SPLITS;
    const int64_t fill = RESIDENT_BLOCKS / row_blocks(n_rows), s = fill > MIN_SPLITS ? fill : MIN_SPLITS;
    return (int)(s > smax ? smax : s);
}

// rows of K_MAX doubles the lists need: splits * n_rows <= max(MIN_SPLITS * n_rows, RESIDENT_BLOCKS * BM), which is monotone (the split count itself is not)
inline int64_t list_rows(int64_t n_rows) {
    const int64_t floor_rows = (int64_t)RESIDENT_BLOCKS * prdc::BM, by_min = MIN_SPLITS * n_rows;
    return by_min > floor_rows ? by_min : floor_rows;
}

inline bool operands_ok(const void* row_planes, const double* row_norms, int64_t n_rows, const void* col_planes, const double* col_norms, int64_t n_cols,
                        int d, int k, int64_t self_offset) {
    return aligned(row_planes, 16) && aligned(col_planes, 16) && aligned(row_norms, 8) && aligned(col_norms, 8) && dims_ok(d, k) && count_ok(n_rows) &&
           count_ok(n_cols) && self_ok(self_offset, n_rows, n_cols) && k + (self_offset >= 0) <= n_cols;
}

inline prdc::Operands operands(const void* row_planes, const double* row_norms, int64_t n_rows, const void* col_planes, const double* col_norms, int64_t n_cols,
                               int d, int64_t self_offset) {
    prdc::Operands op;
    op.a = (const __bf16*)row_planes; op.na = row_norms; op.b = (const __bf16*)col_planes; op.nb = col_norms;
    op.a_plane = n_rows * d; op.b_plane = n_cols * d;
    op.n_rows = (int)n_rows; op.n_cols = (int)n_cols; op.d = d; op.self_offset = self_offset;
    return op;
}

// Column splits of the kernel sums: a function of n_cols alone.  An fp64 sum depends on where the column range is cut, so the cut must not move with the
// number of rows of the call (splits_for's does).  Eight at the most: one column range per XCD, as the radius pass runs at 10,000 rows and more.
constexpr int KID_MAX_SPLITS = MIN_SPLITS;
inline int kid_splits(int64_t n_cols) {
    const int64_t ctiles = (n_cols + prdc::BN - 1) / prdc::BN;
    return (int)(ctiles < KID_MAX_SPLITS ? ctiles : KID_MAX_SPLITS);
}
inline bool stride_ok(int64_t stride, int64_t n, int d) { return stride % 8 == 0 && stride >= n * d; }
inline bool classes_ok(int n_classes) { return n_classes >= 1 && n_classes <= NATINF_IS_MAX_CLASSES; }
inline int64_t staged_row(int n_classes) { return (int64_t)((n_classes + prdc::BN - 1) / prdc::BN) * prdc::BN; }     // doubles per row of staged logits

// ---- the ideal denoiser's staging buffers, one chunk of rows at a time ----
static_assert(NATINF_IDEAL_CHUNK_ROWS >= 64 && NATINF_IDEAL_CHUNK_ROWS % prdc::BM == 0, "a chunk is whole row blocks");
inline int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }
inline int64_t ideal_np(int64_t n_cols) { return (n_cols + 63) / 64 * 64; }
inline int64_t ideal_ranges(int64_t n_cols) { return (ideal_np(n_cols) + prdc::PART_K - 1) / prdc::PART_K; }
struct IdealLayout {
    int64_t R, np, ranges;                                      // rows of the staging buffers (whole row blocks), padded columns, K ranges
    int64_t uplanes, unorms, d2, wplanes, partial, bytes;       // byte offsets into the workspace
};
inline IdealLayout ideal_layout(int64_t n_rows, int64_t n_cols, int d) {
    IdealLayout l;
    const int64_t r64 = row_blocks(n_rows) * prdc::BM;
    l.R = r64 < NATINF_IDEAL_CHUNK_ROWS ? r64 : NATINF_IDEAL_CHUNK_ROWS;
    l.np = ideal_np(n_cols);
    l.ranges = ideal_ranges(n_cols);
    l.uplanes = 0;
    l.unorms = l.uplanes + up256(3 * l.R * d * 2);
    l.d2 = l.unorms + up256(l.R * 8);
    l.wplanes = l.d2 + up256(l.R * n_cols * 8);
    l.partial = l.wplanes + up256(3 * l.R * l.np * 2);
    l.bytes = l.partial + up256(l.ranges * l.R * d * 8);
    return l;
}
inline bool ideal_shape_ok(int64_t n_rows, int64_t n_cols, int d) { return dims_ok(d, 1) && count_ok(n_rows) && count_ok(n_cols); }

// rows [r0, r0 + nr) of the call: planes and norms of the query rows, the d2 chunk, the row stage.  The weight planes are [3][R][np] at ws + wplanes.
inline int ideal_stage(const IdealLayout& l, char* ws, const float* rows, const double* c, int64_t r0, int64_t nr, const void* col_planes,
                       const double* col_norms, int64_t n_cols, int d, int64_t self_offset, double* lse_out, double* pmax_out, int32_t* nearest_out, hipStream_t s)
{
    hipLaunchKernelGGL(prdc::k_prdc_planes, dim3((unsigned)nr), dim3(prdc::THREADS), 0, s, (const float4*)(rows + r0 * d), (prdc::bf16x8*)(ws + l.uplanes),
                       (double*)(ws + l.unorms), d / 8, nr * (d / 8));
    if (launched() != NATINF_OK) return NATINF_ELAUNCH;
    const prdc::Operands op = operands(ws + l.uplanes, (const double*)(ws + l.unorms), nr, col_planes, col_norms, n_cols, d, self_offset >= 0 ? self_offset + r0 : -1);
    const dim3 grid((unsigned)((n_cols + prdc::BN - 1) / prdc::BN), (unsigned)row_blocks(nr));
    hipLaunchKernelGGL(prdc::k_prdc_dist2, grid, dim3(prdc::THREADS), 0, s, op, (double*)(ws + l.d2));
    if (launched() != NATINF_OK) return NATINF_ELAUNCH;
    hipLaunchKernelGGL(ideal::k_ideal_rows, dim3((unsigned)(row_blocks(nr) * prdc::BM)), dim3(64), 0, s, (const double*)(ws + l.d2), (int)nr, (int)n_cols, l.np,
                       c + r0, (__bf16*)(ws + l.wplanes), l.R * l.np, lse_out ? lse_out + r0 : nullptr, pmax_out ? pmax_out + r0 : nullptr,
                       nearest_out ? (int*)nearest_out + r0 : nullptr);
    return launched();
}
}  // namespace

extern "C" {

int64_t natinf_prdc_workspace_bytes(int64_t n_rows, int64_t n_cols, int d, int k)
{
    if (!dims_ok(d, k) || !count_ok(n_rows) || !count_ok(n_cols) || k > n_cols) return NATINF_EINVAL;
    return list_rows(n_rows) * prdc::K_MAX * (int64_t)sizeof(double);
}

int natinf_prdc_planes(const float* feats, int64_t n, int d, void* planes_bf16, double* norms, natinf_stream_t stream)
{
    if (!aligned(feats, 16) || !aligned(planes_bf16, 16) || !aligned(norms, 8) || !count_ok(n) || !dims_ok(d, 1)) return NATINF_EINVAL;
    hipLaunchKernelGGL(prdc::k_prdc_planes, dim3((unsigned)n), dim3(prdc::THREADS), 0, (hipStream_t)stream, (const float4*)feats, (prdc::bf16x8*)planes_bf16,
                       norms, d / 8, n * (d / 8));
    return launched();
}

int natinf_prdc_knn_radius(const void* row_planes, const double* row_norms, int64_t n_rows,
                           const void* col_planes, const double* col_norms, int64_t n_cols,
                           int d, int k, int64_t self_offset, double* r2_out,
                           void* workspace, int64_t workspace_bytes, natinf_stream_t stream)
{
    if (!operands_ok(row_planes, row_norms, n_rows, col_planes, col_norms, n_cols, d, k, self_offset) || !aligned(r2_out, 8) || !aligned(workspace, 256))
        return NATINF_EINVAL;
    if (workspace_bytes < natinf_prdc_workspace_bytes(n_rows, n_cols, d, k)) return NATINF_EINVAL;
    const prdc::Operands op = operands(row_planes, row_norms, n_rows, col_planes, col_norms, n_cols, d, self_offset);
    const int splits = splits_for(n_rows, n_cols);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(prdc::k_prdc_knn, dim3(splits, (unsigned)row_blocks(n_rows)), dim3(prdc::THREADS), 0, s, op, splits, (double*)workspace);
    if (launched() != NATINF_OK) return NATINF_ELAUNCH;
    hipLaunchKernelGGL(prdc::k_prdc_merge, dim3((unsigned)((n_rows + prdc::THREADS - 1) / prdc::THREADS)), dim3(prdc::THREADS), 0, s,
                       (const double*)workspace, n_rows, splits, k, r2_out);
    return launched();
}

int natinf_prdc_ball_counts(const void* row_planes, const double* row_norms, int64_t n_rows,
                            const void* col_planes, const double* col_norms, int64_t n_cols,
                            int d, int64_t self_offset, const double* r2_rows, const double* r2_cols,
                            int32_t* cnt_row_ball, int32_t* cnt_col_ball, natinf_stream_t stream)
{
    if (!operands_ok(row_planes, row_norms, n_rows, col_planes, col_norms, n_cols, d, 1, self_offset)) return NATINF_EINVAL;
    if (!r2_rows != !cnt_row_ball || !r2_cols != !cnt_col_ball || (!cnt_row_ball && !cnt_col_ball)) return NATINF_EINVAL;
    if (((uintptr_t)r2_rows & 7) || ((uintptr_t)r2_cols & 7) || ((uintptr_t)cnt_row_ball & 3) || ((uintptr_t)cnt_col_ball & 3)) return NATINF_EINVAL;
    const prdc::Operands op = operands(row_planes, row_norms, n_rows, col_planes, col_norms, n_cols, d, self_offset);
    const int splits = splits_for(n_rows, n_cols);
    hipStream_t s = (hipStream_t)stream;
    if (cnt_row_ball && hipMemsetAsync(cnt_row_ball, 0, n_rows * sizeof(int32_t), s) != hipSuccess) { (void)hipGetLastError(); return NATINF_ELAUNCH; }
    if (cnt_col_ball && hipMemsetAsync(cnt_col_ball, 0, n_rows * sizeof(int32_t), s) != hipSuccess) { (void)hipGetLastError(); return NATINF_ELAUNCH; }
    hipLaunchKernelGGL(prdc::k_prdc_balls, dim3(splits, (unsigned)row_blocks(n_rows)), dim3(prdc::THREADS), 0, s, op, splits, r2_rows, r2_cols,
                       (int*)cnt_row_ball, (int*)cnt_col_ball);
    return launched();
}

int natinf_prdc_debug_dist2(const void* row_planes, const double* row_norms, int64_t n_rows,
                            const void* col_planes, const double* col_norms, int64_t n_cols,
                            int d, int64_t self_offset, double* d2_out, natinf_stream_t stream)
{
    if (!operands_ok(row_planes, row_norms, n_rows, col_planes, col_norms, n_cols, d, 1, self_offset) || !aligned(d2_out, 8)) return NATINF_EINVAL;
    if (n_rows * n_cols > ((int64_t)1 << 20)) return NATINF_EINVAL;
    const prdc::Operands op = operands(row_planes, row_norms, n_rows, col_planes, col_norms, n_cols, d, self_offset);
    const dim3 grid((unsigned)((n_cols + prdc::BN - 1) / prdc::BN), (unsigned)row_blocks(n_rows));
    hipLaunchKernelGGL(prdc::k_prdc_dist2, grid, dim3(prdc::THREADS), 0, (hipStream_t)stream, op, d2_out);
    return launched();
}

// the column ranges' lists: [list_rows][K_MAX] distances, then as many columns
int64_t natinf_nn_workspace_bytes(int64_t n_rows, int64_t n_cols, int d, int k)
{
    if (!dims_ok(d, k) || !count_ok(n_rows) || !count_ok(n_cols) || k > n_cols) return NATINF_EINVAL;
    return list_rows(n_rows) * prdc::K_MAX * (int64_t)(sizeof(double) + sizeof(int32_t));
}

int natinf_nn_nearest(const void* row_planes, const double* row_norms, int64_t n_rows,
                      const void* col_planes, const double* col_norms, int64_t n_cols,
                      int d, int k, int64_t self_offset, double* d2_out, int32_t* idx_out,
                      void* workspace, int64_t workspace_bytes, natinf_stream_t stream)
{
    if (!operands_ok(row_planes, row_norms, n_rows, col_planes, col_norms, n_cols, d, k, self_offset) || !aligned(d2_out, 8) || !aligned(idx_out, 4) ||
        !aligned(workspace, 256))
        return NATINF_EINVAL;
    if (workspace_bytes < natinf_nn_workspace_bytes(n_rows, n_cols, d, k)) return NATINF_EINVAL;
    static_assert(NATINF_PRDC_MAX_N <= INT32_MAX && prdc::K_MAX == NATINF_PRDC_MAX_K, "natinf_nn.h and prdc.h disagree");
    const prdc::Operands op = operands(row_planes, row_norms, n_rows, col_planes, col_norms, n_cols, d, self_offset);
    const int splits = splits_for(n_rows, n_cols);
    double* lists = (double*)workspace;
    int* cols = (int*)(lists + list_rows(n_rows) * prdc::K_MAX);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(prdc::k_nn_nearest, dim3(splits, (unsigned)row_blocks(n_rows)), dim3(prdc::THREADS), 0, s, op, splits, lists, cols);
    if (launched() != NATINF_OK) return NATINF_ELAUNCH;
    hipLaunchKernelGGL(prdc::k_nn_merge, dim3((unsigned)((n_rows + prdc::THREADS - 1) / prdc::THREADS)), dim3(prdc::THREADS), 0, s,
                       (const double*)lists, (const int*)cols, n_rows, splits, k, d2_out, (int*)idx_out);
    return launched();
}

int64_t natinf_kid_workspace_bytes(int64_t n_rows, int64_t n_cols, int d)
{
    if (!dims_ok(d, 1) || !count_ok(n_rows) || !count_ok(n_cols)) return NATINF_EINVAL;
    return kid_splits(n_cols) * n_rows * (int64_t)sizeof(double);
}

int natinf_kid_row_sums(const void* row_planes, int64_t row_plane_stride, int64_t n_rows,
                        const void* col_planes, int64_t col_plane_stride, int64_t n_cols,
                        int d, int64_t self_offset, double gamma, double coef0,
                        double* sums_out, void* workspace, int64_t workspace_bytes, natinf_stream_t stream)
{
    if (!aligned(row_planes, 16) || !aligned(col_planes, 16) || !dims_ok(d, 1) || !count_ok(n_rows) || !count_ok(n_cols) ||
        !self_ok(self_offset, n_rows, n_cols) || (self_offset >= 0 && n_cols < 2))
        return NATINF_EINVAL;
    if (!stride_ok(row_plane_stride, n_rows, d) || !stride_ok(col_plane_stride, n_cols, d) || !isfinite(gamma) || !isfinite(coef0)) return NATINF_EINVAL;
    if (!aligned(sums_out, 8) || !aligned(workspace, 256) || workspace_bytes < natinf_kid_workspace_bytes(n_rows, n_cols, d)) return NATINF_EINVAL;
    prdc::Operands op = operands(row_planes, nullptr, n_rows, col_planes, nullptr, n_cols, d, self_offset);
    op.a_plane = row_plane_stride; op.b_plane = col_plane_stride;
    const int splits = kid_splits(n_cols);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(prdc::k_kid_sums, dim3(splits, (unsigned)row_blocks(n_rows)), dim3(prdc::THREADS), 0, s, op, splits, gamma, coef0, (double*)workspace);
    if (launched() != NATINF_OK) return NATINF_ELAUNCH;
    hipLaunchKernelGGL(prdc::k_kid_merge, dim3((unsigned)((n_rows + prdc::THREADS - 1) / prdc::THREADS)), dim3(prdc::THREADS), 0, s,
                       (const double*)workspace, n_rows, splits, sums_out);
    return launched();
}

int64_t natinf_is_workspace_bytes(int64_t n_rows, int n_classes, int d)
{
    if (!dims_ok(d, 1) || !count_ok(n_rows) || !classes_ok(n_classes)) return NATINF_EINVAL;
    return (n_rows < NATINF_IS_CHUNK_ROWS ? n_rows : NATINF_IS_CHUNK_ROWS) * staged_row(n_classes) * (int64_t)sizeof(double);
}

int natinf_is_row_stats(const void* row_planes, int64_t row_plane_stride, int64_t n_rows,
                        const void* head_planes, int64_t head_plane_stride, int n_classes, int d,
                        const float* bias, double* neg_entropy_out, double* lse_out, int32_t* top_out, int64_t* class_sums,
                        void* workspace, int64_t workspace_bytes, natinf_stream_t stream)
{
    if (!aligned(row_planes, 16) || !aligned(head_planes, 16) || !dims_ok(d, 1) || !count_ok(n_rows) || !classes_ok(n_classes)) return NATINF_EINVAL;
    if (!stride_ok(row_plane_stride, n_rows, d) || !stride_ok(head_plane_stride, n_classes, d)) return NATINF_EINVAL;
    if (!aligned(neg_entropy_out, 8) || !aligned(class_sums, 8) || ((uintptr_t)lse_out & 7) || ((uintptr_t)top_out & 3) || ((uintptr_t)bias & 3)) return NATINF_EINVAL;
    if (!aligned(workspace, 256) || workspace_bytes < natinf_is_workspace_bytes(n_rows, n_classes, d)) return NATINF_EINVAL;
    static_assert(prdc::IS_MAX_CLASSES == NATINF_IS_MAX_CLASSES && prdc::IS_ONE == (double)((int64_t)1 << NATINF_IS_FRAC_BITS), "natinf_is.h and prdc.h disagree");
    const int64_t ldz = staged_row(n_classes);
    hipStream_t s = (hipStream_t)stream;
    // the rows in chunks through one staging buffer: a chunk's row statistics are enqueued behind its logits, the next chunk's logits behind those
    for (int64_t r0 = 0; r0 < n_rows; r0 += NATINF_IS_CHUNK_ROWS) {
        const int64_t nr = n_rows - r0 < NATINF_IS_CHUNK_ROWS ? n_rows - r0 : NATINF_IS_CHUNK_ROWS;
        prdc::Operands op = operands((const __bf16*)row_planes + r0 * d, nullptr, nr, head_planes, nullptr, n_classes, d, -1);
        op.a_plane = row_plane_stride; op.b_plane = head_plane_stride;
        hipLaunchKernelGGL(prdc::k_is_logits, dim3((unsigned)(ldz / prdc::BN), (unsigned)row_blocks(nr)), dim3(prdc::THREADS), 0, s, op, bias,
                           (double*)workspace);
        if (launched() != NATINF_OK) return NATINF_ELAUNCH;
        hipLaunchKernelGGL(prdc::k_is_rows, dim3((unsigned)((nr + prdc::IS_ROWS - 1) / prdc::IS_ROWS)), dim3(prdc::THREADS), 0, s, (const double*)workspace, ldz,
                           (int)nr, n_classes, neg_entropy_out + r0, lse_out ? lse_out + r0 : nullptr, top_out ? (int*)top_out + r0 : nullptr,
                           (unsigned long long*)class_sums);
        if (launched() != NATINF_OK) return NATINF_ELAUNCH;
    }
    return NATINF_OK;
}

int natinf_ideal_tplanes(const void* planes_bf16, int64_t n, int d, void* tplanes_bf16, natinf_stream_t stream)
{
    if (!aligned(planes_bf16, 16) || !aligned(tplanes_bf16, 16) || !count_ok(n) || !dims_ok(d, 1)) return NATINF_EINVAL;
    const int64_t np = ideal_np(n);
    hipLaunchKernelGGL(ideal::k_ideal_tplanes, dim3((unsigned)(np / ideal::TP), (unsigned)(d / ideal::TP), 3), dim3(prdc::THREADS), 0, (hipStream_t)stream,
                       (const __bf16*)planes_bf16, n, d, np, (__bf16*)tplanes_bf16);
    return launched();
}

int64_t natinf_ideal_workspace_bytes(int64_t n_rows, int64_t n_cols, int d)
{
    if (!ideal_shape_ok(n_rows, n_cols, d)) return NATINF_EINVAL;
    return ideal_layout(n_rows, n_cols, d).bytes;
}

int natinf_ideal_posterior_mean(const float* rows, const double* c, int64_t n_rows,
                                const void* col_planes, const double* col_norms, const void* col_tplanes, int64_t n_cols,
                                int d, int64_t self_offset,
                                const float* x, const double* alpha, const double* sigma,
                                float* x0_out, double* lse_out, double* pmax_out, int32_t* nearest_out, float* out,
                                void* workspace, int64_t workspace_bytes, natinf_stream_t stream)
{
    if (!aligned(rows, 16) || !aligned(c, 8) || !aligned(col_tplanes, 16) || !aligned(x0_out, 4) ||
        !operands_ok(rows, c, n_rows, col_planes, col_norms, n_cols, d, 1, self_offset))
        return NATINF_EINVAL;
    if (((uintptr_t)lse_out & 7) || ((uintptr_t)pmax_out & 7) || ((uintptr_t)nearest_out & 3)) return NATINF_EINVAL;
    if (!x != !alpha || !x != !sigma || !x != !out || ((uintptr_t)x & 3) || ((uintptr_t)out & 3) || ((uintptr_t)alpha & 7) || ((uintptr_t)sigma & 7))
        return NATINF_EINVAL;
    if (!aligned(workspace, 256) || workspace_bytes < natinf_ideal_workspace_bytes(n_rows, n_cols, d)) return NATINF_EINVAL;
    const IdealLayout l = ideal_layout(n_rows, n_cols, d);
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    // a chunk's launches are enqueued behind each other, the next chunk's behind those: one set of staging buffers
    for (int64_t r0 = 0; r0 < n_rows; r0 += NATINF_IDEAL_CHUNK_ROWS) {
        const int64_t nr = n_rows - r0 < NATINF_IDEAL_CHUNK_ROWS ? n_rows - r0 : NATINF_IDEAL_CHUNK_ROWS;
        const int rc = ideal_stage(l, ws, rows, c, r0, nr, col_planes, col_norms, n_cols, d, self_offset, lse_out, pmax_out, nearest_out, s);
        if (rc != NATINF_OK) return rc;
        // mean = W . F on the sweep's tiles: rows = the weight planes, columns = the d rows of the transposed training set, K = np
        prdc::Operands op = operands(ws + l.wplanes, nullptr, nr, col_tplanes, nullptr, d, (int)l.np, -1);
        op.a_plane = l.R * l.np; op.b_plane = (int64_t)d * l.np;
        const dim3 grid((unsigned)((d + prdc::BN - 1) / prdc::BN), (unsigned)row_blocks(nr), (unsigned)l.ranges);
        hipLaunchKernelGGL(ideal::k_ideal_part, grid, dim3(prdc::THREADS), 0, s, op, (double*)(ws + l.partial));
        if (launched() != NATINF_OK) return NATINF_ELAUNCH;
        hipLaunchKernelGGL(ideal::k_ideal_merge, dim3((unsigned)((nr * d + prdc::THREADS - 1) / prdc::THREADS)), dim3(prdc::THREADS), 0, s,
                           (const double*)(ws + l.partial), nr, d, (int)l.ranges, x ? x + r0 * d : nullptr, x ? alpha + r0 : nullptr, x ? sigma + r0 : nullptr,
                           x0_out + r0 * d, out ? out + r0 * d : nullptr);
        if (launched() != NATINF_OK) return NATINF_ELAUNCH;
    }
    return NATINF_OK;
}

int natinf_ideal_debug_weights(const float* rows, const double* c, int64_t n_rows,
                               const void* col_planes, const double* col_norms, int64_t n_cols,
                               int d, int64_t self_offset, float* w_out, void* planes_out,
                               void* workspace, int64_t workspace_bytes, natinf_stream_t stream)
{
    if (!aligned(rows, 16) || !aligned(c, 8) || !aligned(w_out, 4) || ((uintptr_t)planes_out & 15) ||
        !operands_ok(rows, c, n_rows, col_planes, col_norms, n_cols, d, 1, self_offset))
        return NATINF_EINVAL;
    if (n_rows * n_cols > ((int64_t)1 << 20)) return NATINF_EINVAL;
    if (!aligned(workspace, 256) || workspace_bytes < natinf_ideal_workspace_bytes(n_rows, n_cols, d)) return NATINF_EINVAL;
    const IdealLayout l = ideal_layout(n_rows, n_cols, d);
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    for (int64_t r0 = 0; r0 < n_rows; r0 += NATINF_IDEAL_CHUNK_ROWS) {
        const int64_t nr = n_rows - r0 < NATINF_IDEAL_CHUNK_ROWS ? n_rows - r0 : NATINF_IDEAL_CHUNK_ROWS;
        const int rc = ideal_stage(l, ws, rows, c, r0, nr, col_planes, col_norms, n_cols, d, self_offset, nullptr, nullptr, nullptr, s);
        if (rc != NATINF_OK) return rc;
        hipLaunchKernelGGL(ideal::k_ideal_wdebug, dim3((unsigned)((nr * n_cols + prdc::THREADS - 1) / prdc::THREADS)), dim3(prdc::THREADS), 0, s,
                           (const __bf16*)(ws + l.wplanes), l.R * l.np, nr, (int)n_cols, l.np, w_out + r0 * n_cols);
        if (launched() != NATINF_OK) return NATINF_ELAUNCH;
        if (planes_out) {                                       // plane p's rows [r0, r0 + nr) of [3][n_rows][np]
            for (int p = 0; p < 3; ++p)
                if (hipMemcpyAsync((__bf16*)planes_out + (p * n_rows + r0) * l.np, (const __bf16*)(ws + l.wplanes) + p * l.R * l.np, nr * l.np * 2,
                                   hipMemcpyDeviceToDevice, s) != hipSuccess) { (void)hipGetLastError(); return NATINF_ELAUNCH; }
        }
    }
    return NATINF_OK;
}

}  // extern "C"
