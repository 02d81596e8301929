// dit_flash.h -- streaming (flash-style) multi-head attention for the DiT engine at more than 256 tokens (DiT-XL/2 at 512x512: 1,024 tokens,
// head_dim 72).  k_attn_fused keeps all keys of a head in LDS; at 1,024 tokens K and V of a head (padded) are ~360 KB, so here they stream.
//
// One block = 128 queries of one (sample, head): 4 waves x 32 queries.  Keys are walked in tiles of 64; the K tile [64][hd] and the V tile [64][hd]
// of step kt+1 come into LDS by LDS-DMA (global_load_lds, 16 B per lane) while step kt is multiplied (two stages, one barrier per tile).  Scores and
// probabilities stay in registers, no T x T tensor exists anywhere (the operand arrangement of flash_attn.h):
//   S^T = K Q^T        on v_mfma_f32_16x16x32_bf16, the contraction padded to NQK * 32 channels (72 -> 96): Q's padding channels are zero in
//                      registers, so whatever finite K bytes the fragment reads there contribute nothing.  The A-operand rows of S^T tile (2c+h) are
//                      the K rows 32c + 8(r>>2) + 4h + (r&3): a lane then holds keys 32c+8q .. 32c+8q+7 of its query in tiles 2c, 2c+1.
//   online softmax     running max m and per-lane partial sum l per query; exp2 with scale*log2(e) folded into one fma; O rescaled once per tile.
//   O^T = V^T P^T      output padded to ND * 16 channels (72 -> 80).  V stays ROW-MAJOR in LDS (the q | k | v GEMM's layout, DMA'd as it is) and its
//                      A fragments -- eight consecutive keys of one channel -- are read with ds_read_b64_tr_b16 (lo: keys 8q..8q+3, hi: 8q+4..8q+7).
//                      Output channel d depends on V channel d only, so V's padding channels (the next row's bytes) only reach discarded outputs.
// LDS rows: the hd / 8 chunks of 16 B of a row, rounded up to an ODD count RS (64 -> 9, 72 -> 9, 96 -> 13): a 64-row tile is then exactly RS
// DMA wave-instructions of 1 KiB, and 16 consecutive rows start on 16 distinct 16-byte slots of the 256-byte bank row (the fragment reads'
// row order is not consecutive, so some 16-lane groups still share a slot; not measured).  The pad chunk of an even row
// is a copy of the row's last chunk (finite).  The fragment reads of the last rows run up to 112 B past a tile: into the next tile, or the zeroed
// guard behind the second stage.
// Reference: timm Attention as used by deps/DiT/models.py:16,113 (softmax(q k^T * hd^-0.5) v per head).
#pragma once
#include "ncsnpp_kernels.h"

namespace ncsn {

constexpr int DFA_KT = 64, DFA_QB = 128, DFA_GUARD = 256;

struct DitFlashArgs {
    const bf16* q; const bf16* k; const bf16* v; int ld;          // [B*T][ld] each, head h at column h*hd (the engine: one [B*T][3D] buffer)
    bf16* o; int ld_o;                                            // [B*T][ld_o]
    int H, T, hd; float c1;                                       // c1 = hd^-0.5 * log2(e)
};

__host__ __device__ constexpr int dfa_row_chunks(int hd) { return (hd >> 3) | 1; }
inline int dfa_lds_bytes(int hd) { return 4 * dfa_row_chunks(hd) * 1024 + DFA_GUARD; }

// NQK * 32 >= hd (q.k contraction width), ND * 16 >= hd (P.V output width)
template <int NQK, int ND>
__global__ __launch_bounds__(256, 2) void k_dit_flash(const DitFlashArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)             // (the host pass rejects the target builtins of a template body: its stub would be left undefined)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    lds_poison();
    typedef __attribute__((address_space(3))) void lds_void;
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    constexpr int NJ = (2 * (NQK * 4 + 1) + 3) / 4;              // DMA wave-instructions per wave and stage, at most
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int CH = a.hd >> 3, RS = CH | 1, STAGE = RS * 2048;
    const int nQ = a.T / DFA_QB, nK = a.T / DFA_KT;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = tile / nQ, qb = tile - bh * nQ, b = bh / a.H, head = bh - b * a.H;
    const int64_t row0 = (int64_t)b * a.T;
    const bf16* kbase = a.k + row0 * a.ld + head * a.hd;
    const bf16* vbase = a.v + row0 * a.ld + head * a.hd;
    if (tid < DFA_GUARD / 16) *reinterpret_cast<uint4*>(smem + 2 * STAGE + tid * 16) = make_uint4(0u, 0u, 0u, 0u);

    // wave-instruction j of a stage (j = wave + 4 jj) fills LDS [j KiB, j+1 KiB): K for j < RS, V after; its lane's chunk is (row, ch) of the tile
    unsigned off[NJ];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int j = wave + 4 * jj, piece = (j < RS ? j : j - RS) * 64 + lane;
        const int row = piece / RS, ch = min(piece - row * RS, CH - 1);
        off[jj] = (unsigned)(row * a.ld + ch * 8);
    }
    auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
        unsigned char* st = smem + buf * STAGE;
        const int64_t kofs = (int64_t)kt * DFA_KT * a.ld;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = wave + 4 * jj;
            if (j < 2 * RS)
                __builtin_amdgcn_global_load_lds((j < RS ? kbase : vbase) + kofs + off[jj], (lds_void*)(st + j * 1024), 16, 0, 0);
        }
    };
    issue(0, 0);

    bf16x8 qf[2][NQK];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int c = 0; c < NQK; ++c) {
            const int dcol = 32 * c + 8 * q;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (dcol < a.hd) v = *reinterpret_cast<const uint4*>(a.q + (row0 + qb * DFA_QB + wave * 32 + 16 * g + r) * a.ld + head * a.hd + dcol);
            qf[g][c] = __builtin_bit_cast(bf16x8, v);
        }

    float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
    f32x4 oacc[2][ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) { oacc[0][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; oacc[1][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    const int krow = 8 * (r >> 2) + (r & 3);
    const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)smem);
    const unsigned vlane = (unsigned)(((8 * q + (r >> 2)) * RS) * 16 + 8 * (r & 3));      // this lane's transposed-read address inside a 32-key chunk
    for (int kt = 0; kt < nK; ++kt) {
        // tile kt landed (the compiler does not track LDS-DMA completions across the back-edge); the barrier also proves every wave is done with kt-1
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nK) issue(kt + 1, (kt + 1) & 1);
        const unsigned char* sK = smem + (kt & 1) * STAGE;
        const unsigned sV = lds0 + (unsigned)((kt & 1) * STAGE + RS * 1024);

        f32x4 acc[2][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[1][t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int row = 32 * (t >> 1) + 4 * (t & 1) + krow;
#pragma unroll
            for (int c = 0; c < NQK; ++c) {
                const bf16x8 fa = *reinterpret_cast<const bf16x8*>(sK + (row * RS + 4 * c + q) * 16);
                acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, qf[0][c], acc[0][t], 0, 0, 0);
                acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, qf[1][c], acc[1][t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            float mx = m[g];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) mx = fmaxf(mx, acc[g][t][i]);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float alpha = __builtin_amdgcn_exp2f((m[g] - mx) * a.c1), mc = mx * a.c1;      // (first tile: exp2(-inf) = 0)
            m[g] = mx;
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) { const float p = __builtin_amdgcn_exp2f(fmaf(acc[g][t][i], a.c1, -mc)); acc[g][t][i] = p; s += p; }
            l[g] = l[g] * alpha + s;
#pragma unroll
            for (int dt = 0; dt < ND; ++dt)
#pragma unroll
                for (int i = 0; i < 4; ++i) oacc[g][dt][i] *= alpha;
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            bf16x8 pf[2];
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) { pf[g][i] = (bf16)acc[g][2 * c][i]; pf[g][4 + i] = (bf16)acc[g][2 * c + 1][i]; }
            const unsigned va = sV + vlane + (unsigned)(32 * c * RS * 16);
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) {
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(va + 32 * dt));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(va + 32 * dt + 4 * RS * 16));
                const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                const bf16x8 fv = __builtin_bit_cast(bf16x8, both);
                oacc[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv, pf[0], oacc[0][dt], 0, 0, 0);
                oacc[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv, pf[1], oacc[1][dt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        float s = l[g];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const float inv = 1.0f / s;
        bf16* orow = a.o + (row0 + qb * DFA_QB + wave * 32 + 16 * g + r) * a.ld_o + head * a.hd + 4 * q;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
            if (16 * dt + 4 * q < a.hd) {
                typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
                bf16x4 w;
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = (bf16)(oacc[g][dt][i] * inv);
                *reinterpret_cast<bf16x4*>(orow + 16 * dt) = w;
            }
        }
    }
#endif
}

// one instantiation per padded width of the DiT envelope: hd <= 64 -> (64, 64), 72 / 80 -> (96, 80), 88 / 96 -> (96, 96)
inline void launch_dit_flash(const bf16* q, const bf16* k, const bf16* v, int ld, bf16* o, int ld_o, int B, int H, int T, int hd, hipStream_t s)
{
    const DitFlashArgs a{q, k, v, ld, o, ld_o, H, T, hd, 1.4426950408889634f / sqrtf((float)hd)};
    const dim3 grid((unsigned)(B * H * (T / DFA_QB)));
    const int lds = dfa_lds_bytes(hd);
    if (hd <= 64) hipLaunchKernelGGL((k_dit_flash<2, 4>), grid, dim3(256), lds, s, a);
    else if (hd <= 80) hipLaunchKernelGGL((k_dit_flash<3, 5>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((k_dit_flash<3, 6>), grid, dim3(256), lds, s, a);
}

}  // namespace ncsn
