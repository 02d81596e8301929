/*
 * natinf_vae.h -- C ABI of the AutoencoderKL decoder engine inside libnatinf.so (and, at the end, of the encoder engine).
 *
 * Replaces `vae.decode(latents)` at src/ValidateNaturalInference.py:231-236,298-303,366-371 (the step right after the
 * sampling loop).  The reference takes the module from the un-vendored, un-pinned `diffusers`
 * (AutoencoderKL of stabilityai/sd-vae-ft-ema); its arithmetic is restated in oracle/vae_oracle.py from the published
 * architecture (PARITY UNPINNED -- see that file's header) and this engine is tested against that restatement.
 * Decoder: conv_in, mid block (ResnetBlock, single-head attention over the pixels, ResnetBlock), four up blocks of three
 * ResnetBlocks (512, 512, 256, 128 channels; nearest 2x + conv after the first three), GroupNorm + SiLU + conv_out.
 * Latent resolution r is a power of two, 8 <= r <= 64 (the mid-block attention materialises r^2 x r^2 scores per image); the
 * 128x128 latents of SD3 at 1024x1024 need a flash attention at head_dim 512 and are not supported yet.
 *
 * Arithmetic: bf16 operands on the matrix cores, fp32 accumulation, GroupNorm statistics / softmax in fp32.
 */
#ifndef NATINF_VAE_H
#define NATINF_VAE_H

#include <stdint.h>
#include "natinf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct natinf_vae* natinf_vae_t;

int natinf_vae_create(natinf_vae_t* out, int latent_ch, int latent_res);     /* latent_ch 1..64, latent_res 8, 16, 32, 64 or 128 */
int natinf_vae_destroy(natinf_vae_t h);
int64_t natinf_vae_param_count(natinf_vae_t h);
int64_t natinf_vae_packed_bytes(natinf_vae_t h);
int64_t natinf_vae_workspace_bytes(natinf_vae_t h, int max_batch);

/* params_f32: fp32, `post_quant_conv.{weight [C][C], bias}` of the AutoencoderKL (identity / zero if the model has none),
 * then the decoder's parameters in state-dict order of diffusers' `Decoder`:
 *   conv_in.{weight,bias}; mid_block.resnets.0.{norm1.{w,b}, conv1.{w,b}, norm2.{w,b}, conv2.{w,b}};
 *   mid_block.attentions.0.{group_norm.{w,b}, to_q.{w,b}, to_k.{w,b}, to_v.{w,b}, to_out.0.{w,b}}; mid_block.resnets.1.{..};
 *   up_blocks.i.resnets.j.{norm1, conv1, norm2, conv2, [conv_shortcut]} (i = 0..3, j = 0..2), up_blocks.i.upsamplers.0.conv (i < 3);
 *   conv_norm_out.{w,b}; conv_out.{w,b}. */
int natinf_vae_load(natinf_vae_t h, const float* params_f32, int64_t n_params, void* packed, int64_t packed_bytes, natinf_stream_t stream);

/* images = decoder(post_quant_conv(latents)) = AutoencoderKL.decode: latents [B, latent_ch, r, r] fp32 NCHW (already divided
 * by the scaling factor), images [B, 3, 8r, 8r] fp32 NCHW. */
int natinf_vae_decode(natinf_vae_t h, const float* latents, float* images, int B, void* workspace, int64_t workspace_bytes,
                      natinf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * AutoencoderKL ENCODER engine: images -> moments -> latents.  Replaces `vae.encode(images).latent_dist.sample().mul_(0.18215)`
 * at src/AnalyzeWeightedSumDegradation.py:56 (get_feature), and is the first stage of image-to-image / latent inpainting on the
 * DiT and SD3 jobs.  Encoder: conv_in (3 -> 128), four down blocks of two ResnetBlocks (128, 256, 512, 512 channels; a stride-2
 * 3x3 convolution over the input padded by one zero row / column at the bottom / right after the first three), the decoder's
 * mid block, GroupNorm + SiLU + conv_out (512 -> 2*latent_ch), then the AutoencoderKL's 1x1 quant_conv.  Tested against
 * tests/vae_encoder_oracle.py (PARITY UNPINNED, like the decoder's oracle).  Arithmetic as the decoder's.
 *
 * latent_ch 1..32; latent_res r is 8, 16, 32 or 64 (images of 64^2 .. 512^2).  r = 128 (1024^2 images) is refused with
 * NATINF_EINVAL: it is the next size -- its im2col buffer of the first stride-2 convolution and its 1 GiB score matrix per image
 * want a measurement of their own first.
 * ------------------------------------------------------------------------------------------ */
typedef struct natinf_vae_enc* natinf_vae_enc_t;

int natinf_vae_enc_create(natinf_vae_enc_t* out, int latent_ch, int latent_res);
int natinf_vae_enc_destroy(natinf_vae_enc_t h);
int64_t natinf_vae_enc_param_count(natinf_vae_enc_t h);
int64_t natinf_vae_enc_packed_bytes(natinf_vae_enc_t h);
int64_t natinf_vae_enc_workspace_bytes(natinf_vae_enc_t h, int max_batch);

/* params_f32: fp32, the parameters of diffusers' `Encoder` in this order:
 *   conv_in.{weight,bias}; down_blocks.i.resnets.j.{norm1, conv1, norm2, conv2, [conv_shortcut]} (i = 0..3, j = 0..1; channels 128, 256,
 *   512, 512; conv_shortcut where the channel count changes), down_blocks.i.downsamplers.0.conv (i < 3);
 *   mid_block.resnets.0, mid_block.attentions.0.{group_norm, to_q, to_k, to_v, to_out.0}, mid_block.resnets.1 (the decoder's layout);
 *   conv_norm_out.{w,b}; conv_out.{w,b} (512 -> 2*latent_ch);
 * then `quant_conv.{weight [2C][2C], bias}` of the AutoencoderKL (identity / zero if the model has none, as SD3's VAE). */
int natinf_vae_enc_load(natinf_vae_enc_t h, const float* params_f32, int64_t n_params, void* packed, int64_t packed_bytes,
                        natinf_stream_t stream);

/* The posterior of AutoencoderKL.encode on its own (DiagonalGaussianDistribution.sample() / .mode(), then the caller's latent
 * scaling).  moments [n_images, 2*latent_ch, hw] fp32: mean channels first, then logvar.  latents [n_images, latent_ch, hw] fp32.
 * Element e = (c, pixel) of image i, m = that image's moments at that pixel:
 *
 *   logvar = min(max(m[C + c], -30.0f), 20.0f);  std = expf(0.5f * logvar)
 *   z      = sample ? fp32(m[c] + fp32(std * eps)) : m[c]
 *   out    = fp32(fp32(z - shift) * scale)
 *
 * No product and sum is ever fused.  eps is what natinf_randn_philox_col_f32(..., seed, column = NATINF_VAE_POSTERIOR_COLUMN)
 * returns for that image's global index and element, with elems_per_image = C*hw, bit for bit; the global index is image_index[i]
 * (device int64 array) or, when image_index is NULL, first_index + i*index_stride: an image's draw is a function of (seed, global
 * index) only, for any batch split or GPU count.  sample == 0: no draw is made.  The column is disjoint from the noise columns of
 * a matrix (<= N + 1), the inpainting family (2^31 + level) and the colorization family (2^31 + 2^30 + level) for level < 2^29.
 * NATINF_EINVAL, nothing launched: a NULL moments or latents, n_images < 1, latent_ch < 1, hw < 1, C*hw % 4 != 0, C*hw / 4 >= 2^32. */
#define NATINF_VAE_POSTERIOR_COLUMN 0xE0000000u
int natinf_vae_posterior_f32(const float* moments, float* latents, int64_t n_images, int latent_ch, int64_t hw,
                             int sample, float scale, float shift,
                             uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                             natinf_stream_t stream);

/* images [B, 3, 8r, 8r] fp32 NCHW in [-1, 1] -> moments [B, 2*latent_ch, r, r] fp32 NCHW = quant_conv(encoder(images)), what
 * AutoencoderKL.encode builds its DiagonalGaussianDistribution from, and latents [B, latent_ch, r, r] fp32 = the posterior above.
 * Either output may be NULL, not both.  The LAST launch of this call is natinf_vae_posterior_f32's kernel, run on the moments the
 * call has just written (the caller's buffer, or workspace when `moments` is NULL): `latents` equals, byte for byte,
 * natinf_vae_posterior_f32 applied to the `moments` the same call returned.  With latents == NULL that launch is not made.
 * NATINF_EINVAL, nothing launched: a NULL handle or images, both outputs NULL, B < 1, a workspace that is too small, and the
 * posterior's refusals. */
int natinf_vae_encode(natinf_vae_enc_t h, const float* images, float* moments, float* latents, int B,
                      int sample, float scale, float shift,
                      uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                      void* workspace, int64_t workspace_bytes, natinf_stream_t stream);

/* The input passes of the two engines and the encoder's quant_conv alone (tests/test_gpu_glue_kernels.py): the plans' own launchers on caller-supplied device
 * buffers.  Nothing is allocated and nothing waits for the device; every refusal is NATINF_EINVAL with nothing launched.
 * natinf_debug_vae_latents: y bf16 [B][r+2][r+2][64] = post_quant_conv (1x1: W [C][C], bias [C]) of z fp32 [B][C][r][r] in the interior, +0 on the one-pixel
 * border and in the channels >= C.  Refused: a NULL pointer, C outside 1..64, r outside 1..4096, B < 1, 2^31 or more output elements.
 * natinf_debug_vae_images: y bf16 [B][R+2][R+2][64] = img fp32 [B][3][R][R] in channels 0..2 of the interior, +0 elsewhere.  Refused: a NULL pointer, R outside
 * 1..16384, B < 1, 2^31 or more output elements, y not 16-byte aligned.
 * natinf_debug_vae_quant: out[b][c][p] = bias[c] + sum_k W[c][k] m[b][k][p]; m, out fp32 [B][N][hw], W [N][N].  Refused: a NULL pointer, N outside 1..64 (2 *
 * latent_ch of natinf_vae_enc_create), hw < 1, B < 1, 2^31 or more elements. */
int natinf_debug_vae_latents(const float* z, const float* W, const float* bias, void* y, int C, int r, int B, natinf_stream_t stream);
int natinf_debug_vae_images(const float* img, void* y, int R, int B, natinf_stream_t stream);
int natinf_debug_vae_quant(const float* m, const float* W, const float* bias, float* out, int N, int hw, int B, natinf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NATINF_VAE_H */
