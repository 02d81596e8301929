/*
 * natinf_dit.h -- C ABI of the DiT denoiser engine inside libnatinf.so.
 *
 * Replaces `model.forward(zt, timesteps, classlabels)` of src/ValidateNaturalInference.py:190-191, i.e.
 * DiT.forward (deps/DiT/models.py:237-253) with its blocks (:105-146), embedders (:27-99), fixed sin-cos position
 * embedding (:279-326) and unpatchify (:222-235); `timm`'s PatchEmbed / Attention / Mlp (models.py:16) follow their
 * published definitions.  Input size S = 32 (256x256 images, 256 tokens) or 64 (512x512 images, 1,024 tokens), patch 2,
 * 4 input channels, 1000 classes (+1 null), learn_sigma (8 output channels); depth / hidden size / head count and the
 * input size are create-time parameters (DiT-XL/2 = 28 / 1152 / 16).
 *
 * Arithmetic: bf16 operands on the matrix cores, fp32 accumulation, fp32 residual stream, LayerNorm / softmax /
 * modulation in fp32.  Same conventions as natinf.h (device pointers, explicit stream, int return codes, caller-owned
 * packed-weight buffer and workspace).
 */
#ifndef NATINF_DIT_H
#define NATINF_DIT_H

#include <stdint.h>
#include "natinf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct natinf_dit* natinf_dit_t;

/* Attention runs as one fused launch per block when head_dim <= 96 (256 tokens: all keys of a head resident in LDS;
 * 1,024 tokens: keys streamed through LDS, natinf_dit_attention_bf16); this flag selects the per-head GEMM / softmax /
 * GEMM path instead (the one used for larger heads), for testing one against the other. */
#define NATINF_DIT_UNFUSED_ATTENTION 1

/* fp8 projections: per block, the q | k | v, fc1 and fc2 GEMMs run on fp8 e4m3 operands (v_mfma_f32_16x16x128_f8f6f4) with fp32
 * accumulation.
 *   - Their weights are quantised when natinf_dit_load packs them: one fp32 scale per OUTPUT CHANNEL (max |w| / 448), e4m3 bytes.
 *   - The two LayerNorm-modulate passes of a block write e4m3 rows with one fp32 scale per TOKEN (max |h| / 448); the q | k | v and
 *     fc1 GEMMs apply both scales to the fp32 sum in their epilogue.  q | k | v leave that GEMM as bf16 and the attention
 *     (softmax(q k^T) v) runs on bf16 operands exactly as without the flag.
 *   - fc1's epilogue applies the bias and the tanh-GELU in fp32 and writes e4m3 with one E8M0 (power-of-two) scale per 32
 *     columns; fc2 feeds those block scales to the scaled MFMA and applies its weight scales, bias, gate and the residual in
 *     its epilogue.
 *   - Everything else stays bf16: patch embedding, the t / y embedders, the adaLN-modulation GEMM of all blocks, the attention
 *     output projection (its operand is the attention's bf16 output: a quantising pass over it costs what the fp8 GEMM saves,
 *     DESIGN.md section 4b) and the final layer.  The residual stream is as without the flag (natinf_set_dit_stream16).
 * Needs hidden % 128 == 0 (whole 128-byte K-tiles), else NATINF_EINVAL: there is no fallback to bf16.  Combines with
 * NATINF_DIT_UNFUSED_ATTENTION and both input sizes.  natinf_dit_load takes the SAME fp32 parameter vector;
 * natinf_dit_packed_bytes / natinf_dit_workspace_bytes answer for the handle's mode (the packed image is smaller by
 * depth * (11 hidden^2 - 32 hidden) bytes at DiT-XL/2's sizes: 11 hidden^2 matrix bytes saved, 8 hidden scales of 4 bytes added, per block). */
#define NATINF_DIT_FP8 2

/* Stream guard: the residual stream cannot leave the range of its number format unnoticed.  A SITE is one launch of the plan that writes the stream: the patch embedding
 * (site 0), then per block i the attention-projection update (site 1 + 2 i) and the MLP update (site 2 + 2 i): 1 + 2 depth sites.  Each site owns a slot
 * {uint32 max_bits, uint32 clamped} of a status block that lives in the caller's workspace (its first 8 * sites bytes; natinf_dit_workspace_bytes of a guarded handle
 * counts it), and every guarded kernel, with the fp32 result v of an update in hand and before it rounds it:
 *   - tracks max |v|: max_bits = the largest bit pattern of |v| seen (non-negative floats order as unsigned integers; a NaN sorts above +inf and reads back as NaN);
 *   - on a half stream (natinf_set_dit_stream16 = 1) writes |v| > 65504 as +-65504 instead of +-inf and counts it in `clamped` (a NaN stays NaN and is counted);
 *     in range it writes the very bytes the unguarded engine writes.  An fp32 stream is tracked only: `clamped` stays 0 there.
 * The block ACCUMULATES over forwards (max, add; uint32, wrapping) until natinf_dit_stream_status_reset -- nothing else zeroes it, not even the first forward on a fresh
 * workspace -- so one read covers a whole trajectory.  Combines with both other flags, both input sizes and either stream format.  An engine created without the flag runs
 * the kernels it ran before this flag existed.  The flag is bit 4 (16): bits 2 and 3 (4, 8) stay unassigned and NATINF_EINVAL, as callers written against the
 * two-flag library expect of them. */
#define NATINF_DIT_STREAM_GUARD 16

/* hidden % 64 == 0, hidden <= 1536, hidden % heads == 0, (hidden / heads) % 8 == 0; input size 32.  Any flag bit other than the three above: NATINF_EINVAL */
int natinf_dit_create(natinf_dit_t* out, int depth, int hidden, int heads, int flags);
/* the same at input size 32 or 64 (the latent side S: 256 or 1,024 tokens; anything else is NATINF_EINVAL) */
int natinf_dit_create_sized(natinf_dit_t* out, int depth, int hidden, int heads, int input_size, int flags);
int natinf_dit_input_size(natinf_dit_t h);
/* 1 (read when an engine is CREATED): the residual stream x [tokens][hidden] is kept in IEEE half instead of fp32; every update
 * x += gate * (W h + b) is computed in fp32 from the half row and rounded to half once (the MMDiT engine's natinf_set_mmdit_stream16,
 * include/natinf_mmdit.h).  0: fp32; a negative value: the library's default (1 since round 6). */
int natinf_set_dit_stream16(int on);
int natinf_dit_destroy(natinf_dit_t h);
int64_t natinf_dit_param_count(natinf_dit_t h);           /* incl. the frozen pos_embed (tokens x hidden) */
int64_t natinf_dit_packed_bytes(natinf_dit_t h);
int64_t natinf_dit_workspace_bytes(natinf_dit_t h, int max_batch);
/* Guarded handles (NATINF_DIT_STREAM_GUARD); NATINF_EINVAL on any other.  `workspace` is the pointer natinf_dit_forward gets: the block's place in it does not depend on the
 * batch of a forward.  Both calls only enqueue on `stream` (a memset; a device-to-device copy of 2 * sites uint32: {max_bits, clamped} per site, in site order). */
int natinf_dit_stream_sites(natinf_dit_t h);
int natinf_dit_stream_status_reset(natinf_dit_t h, void* workspace, natinf_stream_t stream);
int natinf_dit_stream_status(natinf_dit_t h, const void* workspace, uint32_t* out_dev, natinf_stream_t stream);

/* params_f32: all parameters, fp32, concatenated in this order (reference state-dict names):
 *   pos_embed, x_embedder.proj.{weight,bias}, t_embedder.mlp.0.{weight,bias}, t_embedder.mlp.2.{weight,bias},
 *   y_embedder.embedding_table.weight,
 *   blocks.<i>.{attn.qkv.weight, attn.qkv.bias, attn.proj.weight, attn.proj.bias, mlp.fc1.weight, mlp.fc1.bias,
 *               mlp.fc2.weight, mlp.fc2.bias, adaLN_modulation.1.weight, adaLN_modulation.1.bias}  for i = 0..depth-1,
 *   final_layer.linear.{weight,bias}, final_layer.adaLN_modulation.1.{weight,bias}. */
int natinf_dit_load(natinf_dit_t h, const float* params_f32, int64_t n_params, void* packed, int64_t packed_bytes,
                    natinf_stream_t stream);

/* out = model.forward(z, t, y): z [B,4,S,S] fp32 NCHW (S = the engine's input size), t [B] fp32 timesteps, y [B] int32
 * class labels (1000 = null), out [B,8,S,S] fp32 NCHW. */
int natinf_dit_forward(natinf_dit_t h, const float* z, const float* t, const int32_t* y, float* out, int B,
                       void* workspace, int64_t workspace_bytes, natinf_stream_t stream);

/* The engine's attention alone (tests and measurement): o = softmax(q k^T * hd^-0.5) v per (sample, head), bf16 in and out.
 * q, k, v: [B*T][ld] (head h at columns h*hd .. h*hd+hd-1; the engine passes its one q | k | v buffer, ld = 3 * hidden),
 * o: [B*T][ld_o].  Keys stream through LDS in tiles of 64 (the kernel of 1,024-token engines).  T a multiple of 128 in
 * [256, 4096], hd a multiple of 8 in [8, 96], ld % 8 == 0, ld_o % 4 == 0, q / k / v 16-byte aligned; else NATINF_EINVAL.
 * flags NATINF_DIT_ATTN_RESIDENT: the 256-token kernel instead (all keys of a head in LDS; T must be 256, k addressed
 * as q + (k - q)). */
#define NATINF_DIT_ATTN_RESIDENT 1
int natinf_dit_attention_bf16(const void* q, const void* k, const void* v, int ld, void* o, int ld_o, int B, int T, int H,
                              int hd, int flags, natinf_stream_t stream);

/* The row kernels of the transformer and VAE engines alone (tests): the engines' own launchers on caller-supplied operands.
 *
 * natinf_debug_ln_modulate: h[r][d] = LayerNorm(x[r])[d] * (1 + scale[b][d]) + shift[b][d], b = r / rows_per_sample (no affine,
 * eps 1e-6, biased variance, fp32 statistics).  x: [rows][D] fp32, or IEEE half when x_f16 (read through the same pointer);
 * shift / scale: row b at + b * mod_ld floats.  Exactly one output: h_bf16 [rows][D] bf16 (launch_ln_modulate), or h_fp8
 * [rows][D] e4m3 bytes with row_scale [rows] (launch_ln_modulate<RowsFp8>: row_scale = max|h[r]| / 448, 1.0 for an all-zero
 * row; bytes = e4m3(h / row_scale), round to nearest even, clamped to +-448).  *form_out: the kernel form the launcher chose,
 * 0 scalar (any D, any alignment), 1 four columns per lane (D 256 / 1152 / 1536; D 256 / 1152 on the half stream), 2 eight
 * columns per lane (D 1536 on the half stream); the vector forms need mod_ld % 4 == 0 and 16-byte aligned shift / scale.
 * NATINF_EINVAL, nothing launched: a NULL x / shift / scale / form_out; both outputs or neither (h_fp8 and row_scale go
 * together); D <= 0, D > 1536, D % 64 (fp8: D % 128); rows <= 0; rows_per_sample <= 0; mod_ld < D; x or the output not
 * 16-byte aligned. */
int natinf_debug_ln_modulate(const void* x, int x_f16, const float* shift, const float* scale, int mod_ld, void* h_bf16, void* h_fp8,
                             float* row_scale, int D, int64_t rows, int rows_per_sample, int* form_out, natinf_stream_t stream);
/* P[r] = softmax(S[r]): S fp32 [rows][T] -> P bf16 [rows][T], one wave per row, with the engines' grid and block.
 * kind 0 k_softmax_rows (T <= 256, T % 4 == 0 or T == 16), 1 k_softmax_rows_1k (T % 64 == 0, T <= 1024), 2
 * k_softmax_rows_wide (T % 64 == 0).  NATINF_EINVAL, nothing launched: a NULL S / P, kind outside 0..2, rows <= 0, T <= 0 or
 * outside the kind's contract. */
int natinf_debug_softmax_rows(int kind, const float* S, void* P, int T, int64_t rows, natinf_stream_t stream);

/* The glue kernels at the two ends of the DiT and SD3-MMDiT engines alone (tests/test_gpu_glue_kernels.py): the plans' own launchers on caller-supplied device
 * buffers.  Nothing is allocated and nothing waits for the device; every refusal below is NATINF_EINVAL with nothing launched.
 *
 * natinf_debug_patch_embed: x[b*g*g + t][d] = sum_k w[d][k] patch(b, t)[k] + bias[d] + pos[t][d], k = (c, pi, qi) as Conv2d(C, D, 2, stride 2) flattens its
 * weight.  z [B][C][2g][2g] fp32; w [D][C*4] fp32, the conv weight as a checkpoint stores it; wt: scratch of D*C*4 floats that receives its transpose [C*4][D]
 * (k_transpose_f32, as the engines' load does), which the embedding kernel then reads; bias [D]; pos [g*g][D]; x [B*g*g][D] fp32, or IEEE half when x_f16.
 * guard: NULL, or a status slot {uint32 max_bits, uint32 clamped} (NATINF_DIT_STREAM_GUARD above): the guarded kernel instances, which accumulate into the slot.
 * Refused: a NULL z / w / wt / bias / pos / x; C outside 1..16; g outside 1..256; D outside 64..1536 or D % 64; B < 1; more than 65535 * 16 rows; x not aligned to
 * its element; guard not 4-byte aligned.
 * natinf_debug_dit_time_freq: emb [B][256] bf16 = [cos(t f_h) | sin(t f_h)], f_h = exp(-ln(1e4) h / 128), h = 0..127.  Refused: NULL t / emb, B outside 1..2^22.
 * natinf_debug_dit_cond: cs[b][d] = bf16(SiLU(c0[b][d] + table[y[b]][d])); c0 [B][D] fp32, table [classes][D] fp32, y [B] int32 (device; not range-checked).
 * Refused: a NULL pointer, D < 1, B < 1, B * D >= 2^31.
 * natinf_debug_silu_bf16: cs[i] = bf16(SiLU(c[i])); natinf_debug_f32_to_bf16: dst[i] = bf16(src[i]), round to nearest even.  Refused: a NULL pointer, n < 1, n >= 2^31.
 * natinf_debug_unpatchify: out[n][c][2 gh + pi][2 gw + qi] = tok[n*g*g + gh*g + gw][(2 pi + qi) * OC + c]; tok [n_images*g*g][4*OC] fp32, out [n_images][OC][2g][2g]
 * fp32.  Refused: a NULL pointer, OC or g outside 1..4096, n_images < 1, 2^31 or more elements. */
int natinf_debug_patch_embed(const float* z, const float* w, float* wt, const float* bias, const float* pos, void* x, int x_f16, uint32_t* guard,
                             int C, int g, int D, int B, natinf_stream_t stream);
int natinf_debug_dit_time_freq(const float* t, void* emb, int B, natinf_stream_t stream);
int natinf_debug_dit_cond(const float* c0, const float* table, const int32_t* y, void* cs, int D, int B, natinf_stream_t stream);
int natinf_debug_silu_bf16(const float* c, void* cs, int64_t n, natinf_stream_t stream);
int natinf_debug_f32_to_bf16(const float* src, void* dst, int64_t n, natinf_stream_t stream);
int natinf_debug_unpatchify(const float* tok, float* out, int OC, int g, int n_images, natinf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NATINF_DIT_H */
