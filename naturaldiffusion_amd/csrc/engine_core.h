// engine_core.h -- what every engine (NCSN++, DiT, MMDiT, VAE decoder, Inception) is built on: the per-forward launch context, the
// workspace arena, the engine base (a launch plan over a packed-weight image) and the plan builder's shared recipes.  Part of the one
// translation unit ncsnpp.hip; the GEMM launch layer the ops call is gemm_launch.h.  What only the transformer plans share (Lin / Lin8, the builder
// base that takes and packs a Linear, the GEMM recipes) is transformer_plan.h.
#pragma once
#include <functional>
#include <map>
#include <vector>

#include "natinf_ncsnpp.h"
#include "gemm_launch.h"

namespace ncsn {

// dst[k][n] = src[n][k]   (bytes checked through natinf_debug_patch_embed's scratch: tests/test_gpu_glue_kernels.py)
__global__ void k_transpose_f32(const float* __restrict__ src, float* __restrict__ dst, int N, int K)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * K) return;
    const int n = (int)(i / K), k = (int)(i - (int64_t)n * K);
    dst[(int64_t)k * N + n] = src[i];
}
}  // namespace ncsn

namespace {

inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
// src [rows][cols] -> dst [cols][rows]: a plan's load-time transpose (PlanBuilder::pack_f32_transposed) and natinf_debug_patch_embed (dit_engine.inc) launch it here
inline void launch_transpose_f32(const float* src, float* dst, int rows, int cols, hipStream_t s) {
    const int64_t n = (int64_t)rows * cols;
    hipLaunchKernelGGL(k_transpose_f32, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, s, src, dst, rows, cols);
}

// tensor reference inside the workspace: `off` is BYTES PER IMAGE (actual = off * B)
// coff: channel offset inside a wider buffer; pad = 1: stored with a one-pixel zero border (3x3 GEMM inputs)
struct TRef { int64_t off = -1; int C = 0, ld = 0, res = 0, coff = 0, pad = 0; };

struct Ctx {                     // per-forward launch context
    int B; unsigned char* ws; const unsigned char* wp; hipStream_t stream;
    const float* x; const float* labels; float* out;
    int* part_bm;                // [n_parts] block-tile rows (BM) of the GEMM variant that wrote each partial table
    hipStream_t stream2 = nullptr; hipEvent_t* ev = nullptr;      // MMDiT engine: the text stream's own HIP stream and the fork / join events (null: everything on `stream`)
    unsigned char* fin_done = nullptr;   // [n_parts] per FORWARD, like part_bm: the launch that wrote partial table i also wrote its consumer's GroupNorm table (see Fin).  Not plan
                                         // state: a description pass (scratch array) or a second thread's forward on a shared plan cannot flip it under a running forward
    uint32_t* guard = nullptr;           // guarded transformer engines: the status block {max_bits, clamped} x sites at the head of the caller's workspace (EngineCore::guard_sites); null = unguarded
    uint32_t* site(int i) const { return guard ? guard + 2 * i : nullptr; }      // GemmArgs::stream_guard of stream-writing launch i of the plan
    bf16* act(const TRef& t) const { return reinterpret_cast<bf16*>(ws + t.off * B) + t.coff; }
    template <class T> T* at(int64_t off) const { return reinterpret_cast<T*>(ws + off * B); }
    template <class T> const T* w(int64_t off) const { return reinterpret_cast<const T*>(wp + off); }
};
using OpFn = std::function<void(const Ctx&)>;

struct PackCtx { const float* params; unsigned char* packed; hipStream_t stream; };
using PackFn = std::function<void(const PackCtx&)>;

// first-fit arena over "bytes per image"
struct Arena {
    bool keep = false; int64_t top = 0, peak = 0;
    std::map<int64_t, int64_t> free_;      // off -> size
    std::map<int64_t, int64_t> live_;
    int64_t alloc(int64_t bytes) {
        bytes = align_up(bytes, 256);
        if (!keep)
            for (auto it = free_.begin(); it != free_.end(); ++it)
                if (it->second >= bytes) {
                    const int64_t off = it->first, rest = it->second - bytes;
                    free_.erase(it);
                    if (rest) free_[off + bytes] = rest;
                    live_[off] = bytes;
                    return off;
                }
        const int64_t off = top; top += bytes; if (top > peak) peak = top;
        live_[off] = bytes;
        return off;
    }
    void release(int64_t off) {
        if (keep || off < 0) return;
        auto it = live_.find(off);
        if (it == live_.end()) return;
        int64_t o = off, s = it->second;
        live_.erase(it);
        auto nx = free_.lower_bound(o);
        if (nx != free_.end() && o + s == nx->first) { s += nx->second; nx = free_.erase(nx); }
        if (nx != free_.begin()) { auto pv = std::prev(nx); if (pv->first + pv->second == o) { o = pv->first; s += pv->second; free_.erase(pv); } }
        if (o + s == top) top = o; else free_[o] = s;
    }
};

}  // namespace

struct EngineCore {                      // what an engine is: a launch plan over a packed-weight image
    int64_t n_params = 0, packed_bytes = 0, ws_per_image = 0;
    std::vector<OpFn> ops;
    std::vector<PackFn> packs;
    const unsigned char* packed = nullptr;
    bool configured = false;
    std::vector<int> part_bm{128};
    // Stream guard (NATINF_DIT_STREAM_GUARD / NATINF_MMDIT_STREAM_GUARD): guard_sites stream-writing launches, each with a slot {uint32 max_bits, uint32 clamped} in a status
    // block of guard_bytes() at the HEAD of the caller's workspace -- in front of the arena, whose offsets scale with the batch of a forward, so that the block is where
    // it is for any batch size and the status entries need the workspace pointer only.  Forwards accumulate into it (atomic max / add); nothing zeroes it but status_reset.
    int guard_sites = 0;
    int64_t guard_bytes() const { return guard_sites ? align_up((int64_t)guard_sites * 8, 256) : 0; }
    int64_t workspace_bytes(int max_batch) const { return ws_per_image * (int64_t)max_batch + guard_bytes(); }
    int status_reset(void* ws, hipStream_t s) const {
        if (!guard_sites || !ws) return NATINF_EINVAL;
        return hipMemsetAsync(ws, 0, (size_t)guard_sites * 8, s) == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
    }
    int status_read(const void* ws, uint32_t* out_dev, hipStream_t s) const {
        if (!guard_sites || !ws || !out_dev) return NATINF_EINVAL;
        return hipMemcpyAsync(out_dev, ws, (size_t)guard_sites * 8, hipMemcpyDeviceToDevice, s) == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
    }
    int load(const float* params_f32, int64_t n, void* dst, int64_t dst_bytes, hipStream_t s) {
        if (!params_f32 || !dst || n != n_params || dst_bytes < packed_bytes) return NATINF_EINVAL;
        PackCtx p{params_f32, reinterpret_cast<unsigned char*>(dst), s};
        for (const auto& f : packs) f(p);
        packed = reinterpret_cast<const unsigned char*>(dst);
        return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
    }
    int run(const float* x, const float* t, float* out, int B, void* ws, int64_t ws_bytes, hipStream_t s, hipStream_t s2 = nullptr, hipEvent_t* ev = nullptr) {
        if (!x || !t || !out || !ws || B <= 0) return NATINF_EINVAL;
        if (!packed) return NATINF_ESTATE;
        if (ws_bytes < workspace_bytes(B)) return NATINF_EINVAL;
        if (!configured) { if (!configure_gemm_kernels()) return NATINF_ENODEV; configured = true; }
        Ctx c{B, reinterpret_cast<unsigned char*>(ws) + guard_bytes(), packed, s, x, t, out, part_bm.data()};
        c.stream2 = s2; c.ev = ev;
        if (guard_sites) { c.guard = reinterpret_cast<uint32_t*>(ws); g_launch_error = 0; }
        for (const auto& f : ops) f(c);
        if (guard_sites && g_launch_error) { g_launch_error = 0; return NATINF_ESTATE; }      // a guarded site whose launch has no guarded kernel: refused, not written unguarded
        return hipGetLastError() == hipSuccess ? NATINF_OK : NATINF_ELAUNCH;
    }
};

namespace {

struct PlanBuilder {
    EngineCore& E;
    Arena arena;
    int64_t wtop = 0, poff = 0;
    explicit PlanBuilder(EngineCore& e) : E(e) {}
    int64_t wres(int64_t bytes) { const int64_t o = wtop; wtop += align_up(bytes, 256); return o; }
    int64_t take(int64_t n) { const int64_t o = poff; poff += n; return o; }
    void op(OpFn f) { E.ops.push_back(std::move(f)); }
    int64_t pack_bf16(int64_t src, int rows, int cols) {             // [rows][cols] fp32 -> bf16, same layout
        const int64_t dst = wres((int64_t)rows * cols * 2);
        E.packs.push_back([=](const PackCtx& p) {
            const int64_t n = (int64_t)rows * cols;
            hipLaunchKernelGGL(k_pack_conv, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream, p.params + src,
                               reinterpret_cast<bf16*>(p.packed + dst), rows, cols, 1, cols, 0, cols, 0, 1.0f);
        });
        return dst;
    }
    void pack_bf16_at(int64_t src, int rows, int cols, int64_t dst) {
        E.packs.push_back([=](const PackCtx& p) {
            const int64_t n = (int64_t)rows * cols;
            hipLaunchKernelGGL(k_pack_conv, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream, p.params + src,
                               reinterpret_cast<bf16*>(p.packed + dst), rows, cols, 1, cols, 0, cols, 0, 1.0f);
        });
    }
    int64_t pack_f32(int64_t src, int64_t n, int64_t src2 = -1) {      // returns the packed offset of an fp32 vector
        const int64_t dst = wres(n * 4);
        pack_f32_at(src, n, dst, src2);
        return dst;
    }
    int64_t pack_f32_transposed(int64_t src, int rows, int cols) {     // [rows][cols] -> [cols][rows]
        const int64_t dst = wres((int64_t)rows * cols * 4);
        E.packs.push_back([=](const PackCtx& p) { launch_transpose_f32(p.params + src, reinterpret_cast<float*>(p.packed + dst), rows, cols, p.stream); });
        return dst;
    }
    void pack_f32_at(int64_t src, int64_t n, int64_t dst, int64_t src2 = -1) {      // src2: a second vector added to the first (the NCSN++ summed shortcut bias)
        E.packs.push_back([=](const PackCtx& p) {
            hipLaunchKernelGGL(k_copy_add_f32, dim3(grid1d(n, 256, 1 << 30)), dim3(256), 0, p.stream, p.params + src,
                               src2 >= 0 ? p.params + src2 : (const float*)nullptr, reinterpret_cast<float*>(p.packed + dst), (int)n);
        });
    }

    void pack_fp8_at(int64_t src, int rows, int cols, int64_t wdst, int64_t sdst) {      // [rows][cols] fp32 -> e4m3 bytes, same layout, + one fp32 scale per row (output channel)
        E.packs.push_back([=](const PackCtx& p) {
            hipLaunchKernelGGL(k_pack_fp8_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, p.stream, p.params + src,
                               reinterpret_cast<uint8_t*>(p.packed + wdst), reinterpret_cast<float*>(p.packed + sdst), rows, cols);
        });
    }

    void finish() { E.n_params = poff; E.packed_bytes = wtop; E.ws_per_image = arena.peak; }
};

}  // namespace
