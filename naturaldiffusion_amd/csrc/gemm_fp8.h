// gemm_fp8.h -- 256x256x128 LDS-DMA GEMM on fp8 (e4m3) operands: k_gemm_fp8.
//
// C[m][n] = deq_m[m] * deq_n[n] * sum_k A8[m][k] * B8[n][k]  (+ the usual epilogue terms), A8 / B8 row-major fp8 bytes
// with one fp32 scale per row (activations: per token, written by the LayerNorm-modulate kernels' RowsFp8 policy,
// transformer_rows.h; weights: per output channel, written at load time by k_pack_fp8_rows below).  A K-tile is 128 bytes per row -- the SAME LDS image, DMA pieces and swizzle as the bf16 kernel's 64-wide
// tiles -- but it feeds v_mfma_f32_16x16x128_f8f6f4 (a lane supplies 32 K bytes of its row: two 16-byte LDS
// reads), which does four times the K of the bf16 MFMA in twice its time: twice the flops per byte moved and per cycle.
// Unit block scales in the MFMA (127 = 2^0); the real scales are applied once, in the epilogue.
// Two-stage pipeline like k_gemm_dma<2,4,8,4> (one K-tile of prefetch, explicit vmcnt(0) + barrier per K-tile), swapped
// operands, slab epilogue.  Plain GEMMs only (taps = 1, one K segment); K % 128 == 0; M / N edges clamped.
#pragma once
#include "gemm_dma.h"

namespace ncsn {

typedef int i32x8 __attribute__((ext_vector_type(8)));

// EPI (chosen on the host, launch_gemm_fp8): 0 = fp32-slab epilogue; 1 = packed bf16 output (row / column scales, biases);
// 2 = packed e4m3 + E8M0 output with tanh-GELU (fc1 -> fc2's operand); 3 = direct fp32 residual-stream epilogue.
template <bool MXA, int EPI = 0>     // MXA: the A operand carries E8M0 block scales (GemmArgs::a_mx), fed to the MFMA lane by lane
__global__ __launch_bounds__(512, 2) void k_gemm_fp8(const GemmArgs g)
{
    using Cfg = DmaCfg<2, 4, 8, 4>;
    constexpr int WN = 4, TM = 8, TN = 4, BM_ = 256, BN_ = 256, BKB = 128;       // BKB: K bytes (= elements) per tile
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    lds_poison();
    typedef __attribute__((address_space(3))) void lds_void;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int nN = (g.N + BN_ - 1) / BN_, nM = (g.M + BM_ - 1) / BM_;
    const int tile = xcd_remap(blockIdx.x, nM * nN);
    int mt_, nt_;
    tile_coords(tile, nM, nN, g.raster_g, mt_, nt_);
    const int m0 = mt_ * BM_, n0 = nt_ * BN_;
    const int z = blockIdx.z;
    const uint8_t* a0 = reinterpret_cast<const uint8_t*>(g.a0) + (int64_t)z * g.a_bs;     // strides in bytes = elements
    const uint8_t* bp = reinterpret_cast<const uint8_t*>(g.b) + (int64_t)z * g.b_bs;
    const int nk = g.a0_C / BKB;

    // one wave per SIMD (waves 0..3) issues all LDS-DMA pieces, two waves' worth each (see k_gemm_dma SPREAD 6)
    constexpr int PAI = 2 * Cfg::PA, PBI = 2 * Cfg::PB;
    const bool issuer = wave < Cfg::NW / 2;
    uint64_t a_row[PAI], b_row[PBI];
#pragma unroll
    for (int j = 0; j < PAI; ++j) {
        const int r = (wave * PAI + j) * 8 + (lane >> 3);
        a_row[j] = reinterpret_cast<uint64_t>(a0 + (int64_t)min(m0 + r, g.M - 1) * g.a0_ld + (((lane & 7) ^ ((r >> 1) & 7)) << 4));
    }
#pragma unroll
    for (int j = 0; j < PBI; ++j) {
        const int r = (wave * PBI + j) * 8 + (lane >> 3);
        b_row[j] = reinterpret_cast<uint64_t>(bp + (int64_t)min(n0 + r, g.N - 1) * g.b_ld + (((lane & 7) ^ ((r >> 1) & 7)) << 4));
    }
    auto issue_tile = [&](int kt, int buf) __attribute__((always_inline)) {
        if (!issuer) return;
        unsigned char* dA = smem + buf * Cfg::STAGE_BYTES + wave * (PAI * 1024);
        unsigned char* dB = smem + buf * Cfg::STAGE_BYTES + BM_ * 128 + wave * (PBI * 1024);
#pragma unroll
        for (int j = 0; j < PAI; ++j)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(a_row[j] + (uint64_t)kt * BKB), (lds_void*)(dA + j * 1024), 16, 0, 0);
#pragma unroll
        for (int j = 0; j < PBI; ++j)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(b_row[j] + (uint64_t)kt * BKB), (lds_void*)(dB + j * 1024), 16, 0, 0);
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4, fswz = (frow >> 1) & 7;
    // MX scales of the A rows: stored K-TILE MAJOR (ncsnpp_kernels.h), so the 256 rows x 4 blocks of one K-tile are 1 KiB
    // of consecutive bytes -- one more DMA piece per stage (wave 0), parked behind the operand stages.  A lane then reads
    // the dword of each of its rows from LDS and uses byte fq.  (Plain per-lane loads of the scales in the K loop cost
    // 35 % of the kernel: they share vmcnt with the DMA and sit on the critical path.)
    unsigned sc[TM];
    const uint8_t* mx_src = MXA ? g.a_mx + (int64_t)z * g.a_mx_bs + (int64_t)m0 * 4 + lane * 16 : nullptr;
    auto issue_mx = [&](int kt, int buf) __attribute__((always_inline)) {
        if (wave == 0)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(mx_src + (int64_t)kt * g.a_mx_ld * 4), (lds_void*)(smem + 131072 + buf * 1024), 16, 0, 0);
    };
    if constexpr (MXA) issue_mx(0, 0);
    issue_tile(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // The MFMA's K order (probed, tools/fp8_probe): lane group q supplies K bytes 16q..16q+15 in its first four registers
    // and 64+16q..64+16q+15 in the other four -- two stacked 64-wide halves -- and MX block j (K bytes 32j..32j+31) takes
    // its scale from lane group j.  So a lane reads the 16-byte chunks q and 4+q of its row (not 2q, 2q+1): memory-
    // contiguous 32-blocks are then the hardware's blocks.  (Without block scales any order common to A and B would do.)
    const int c0 = (fq ^ fswz) << 4, c1 = ((4 + fq) ^ fswz) << 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) issue_tile(kt + 1, cur ^ 1);
        if constexpr (MXA) {
            if (kt + 1 < nk) issue_mx(kt + 1, cur ^ 1);
#pragma unroll
            for (int i = 0; i < TM; ++i)
                sc[i] = (*reinterpret_cast<const unsigned*>(smem + 131072 + cur * 1024 + (wm * TM * 16 + i * 16 + frow) * 4) >> (8 * fq)) & 0xffu;
        }
        const unsigned char* ta = smem + cur * Cfg::STAGE_BYTES + (wm * TM * 16 + frow) * 128;
        const unsigned char* tb = smem + cur * Cfg::STAGE_BYTES + BM_ * 128 + (wn * TN * 16 + frow) * 128;
        i32x8 fb[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const uint4 lo = *reinterpret_cast<const uint4*>(tb + j * 2048 + c0), hi = *reinterpret_cast<const uint4*>(tb + j * 2048 + c1);
            fb[j] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const uint4 lo = *reinterpret_cast<const uint4*>(ta + i * 2048 + c0), hi = *reinterpret_cast<const uint4*>(ta + i * 2048 + c1);
            const i32x8 fa = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[j], fa, acc[i][j], 0, 0, 0, 127, 0, MXA ? (int)sc[i] : 127);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if constexpr (EPI == 1) packed_tile_epilogue<2, 4, 8, 4, typename Cfg::Epi, ACT_NONE, false, false, true, false>(g, smem, acc, m0, n0, z, tid, lane, wm, wn);
    else if constexpr (EPI == 2) packed_tile_epilogue<2, 4, 8, 4, typename Cfg::Epi, ACT_GELU_TANH, false, false, true, true>(g, smem, acc, m0, n0, z, tid, lane, wm, wn);
    else if constexpr (EPI == 3) direct_f32_epilogue<2, 4, 8, 4, true>(g, acc, m0, n0, z, lane, wm, wn);
    // 3 guarded (GemmArgs::stream_guard).  One residual row-tile in flight instead of two: with two, the guard's two accumulators and its constants cost this 256-register
    // kernel five spilled registers; the arithmetic per value is the same
    else if constexpr (EPI == 4) direct_f32_epilogue<2, 4, 8, 4, true, 1, true>(g, acc, m0, n0, z, lane, wm, wn);
    else dma_tile_epilogue<2, 4, 8, 4, typename Cfg::Epi>(g, smem, acc, m0, n0, z, tid, lane, wm, wn);
}

// weights: W fp32 [N][K] -> fp8 bytes [N][K] + one scale per output channel
__global__ __launch_bounds__(256) void k_pack_fp8_rows(const float* __restrict__ W, uint8_t* __restrict__ q, float* __restrict__ row_scale, int N, int K)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float* w = W + (int64_t)row * K;
    float amax = 0.f;
    for (int k = lane; k < K; k += 64) amax = fmaxf(amax, fabsf(w[k]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    const float qs = amax > 0.f ? amax / 448.0f : 1.0f, inv = 1.0f / qs;
    if (lane == 0) row_scale[row] = qs;
    for (int k = 2 * lane; k < K; k += 128) {
        const float a = fminf(fmaxf(w[k] * inv, -448.f), 448.f), c = fminf(fmaxf(w[k + 1] * inv, -448.f), 448.f);
        *reinterpret_cast<uint16_t*>(q + (int64_t)row * K + k) = (uint16_t)(__builtin_amdgcn_cvt_pk_fp8_f32(a, c, 0, false) & 0xffff);
    }
}

}  // namespace ncsn
