/*
 * natinf_inception.h -- C ABI of the FID Inception-V3 pool3 engine inside libnatinf.so.
 *
 * Replaces `InceptionV3([BLOCK_INDEX_BY_DIM[2048]])(batch)[0]` in the reference's FID epilogue -- get_activation / calc_fid,
 * src/CIFAR10NaturalInference.py:44-86: uint8 HWC images / 255 -> NCHW -> pool3 features [n, 2048] -> (mean, covariance) -> Frechet
 * distance (naturaldiffusion_amd/fid_stats.py).  The reference takes the module from un-vendored, un-pinned `pytorch_fid`
 * (a subclass of torchvision's Inception3 with three FID patches); its arithmetic is restated in oracle/inception_oracle.py from the
 * published architecture (PARITY UNPINNED -- see that file's header) and this engine is tested against that restatement.
 * Network: bilinear resize to 299x299 (align_corners = False), 2x - 1, Conv2d_1a .. Conv2d_4a with two 3x3 / stride-2 max pools,
 * Mixed_5b-5d (FIDInceptionA), Mixed_6a, Mixed_6b-6e (FIDInceptionC), Mixed_7a, Mixed_7b (FIDInceptionE_1), Mixed_7c (FIDInceptionE_2),
 * global average pool.  BatchNorm (eval, eps 1e-3) is folded into the filters when the weights are packed.
 *
 * Arithmetic (default plan; natinf_set_inception_conv below): IEEE-half operands on the matrix cores -- activations, and filters as one half-precision term per
 * power-of-two-scaled row --, fp32 accumulation, column scale + bias + ReLU in fp32, activations stored as half; features fp32.  Plans 0 / 1: bf16 operands, filters as
 * two bf16 terms, activations stored as bf16.
 */
#ifndef NATINF_INCEPTION_H
#define NATINF_INCEPTION_H

#include <stdint.h>
#include "natinf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct natinf_inception* natinf_inception_t;

enum { NATINF_INCEPTION_U8_HWC = 0,     /* images: uint8 [B][H][W][3], the tensor the reference's samplers produce (to_pixel) */
       NATINF_INCEPTION_F32_CHW = 1 };  /* images: fp32 [B][3][H][W] in [0, 1], what the reference hands to the module */

int natinf_inception_create(natinf_inception_t* out, int in_h, int in_w);    /* input image size (32 x 32 for CIFAR10) */
int natinf_inception_destroy(natinf_inception_t h);
/* A/B switch, read by natinf_inception_create: 2 (default) = every convolution is one implicit-GEMM launch (csrc/conv_ring.h: the activation tensor is the A
 * operand, a K-tile = one tap x 32 channels) on HALF-PRECISION activations and one half-precision filter term (rows scaled by a power of two); 1 = the same launches
 * on bf16 activations with the filters as two bf16 terms; 0 = the round-3 / 4 plan (bf16, two terms, an im2col pass + a GEMM per convolution).  The parameter order
 * and the features' meaning are the same; packed_bytes / workspace_bytes differ (ask the handle). */
int natinf_set_inception_conv(int mode);
/* The engine's convolution kernel on caller-supplied operands (tests): out[b, oy, ox, n] = relu(col_scale[n] * sum_{ky, kx, c} x[b, oy*stride - ph + ky, ox*stride - pw + kx, c]
 * * w[n, (ky*kw + kx)*cin_p + c] + bias[n]), zero padding.  x: 16-bit [B][H][W][x_ld] (bf16, or IEEE half when f16 = 1), cin_p % 32 == 0 channels read per pixel;
 * w_packed: 16-bit [cout][passes * kh*kw*cin_p] (passes = 2: the second block of columns is a second filter term over the same taps); bias / col_scale: fp32 [cout] or NULL;
 * zeros: >= 16 zero bytes on the device (what padding taps fetch); out: 16-bit [B*Ho*Wo][out_ld], cout % 8 == 0.  tile: 0 = 256 x 64, 1 = 256 x 128, 2 = 128 x 128,
 * 3 = 128 x 192 (f16 only). */
int natinf_debug_conv_ring(int tile, int f16, int B, int H, int W, int cin_p, int x_ld, int cout, int kh, int kw, int stride, int ph, int pw, int passes,
                           const void* x, const void* w_packed, const float* bias, const float* col_scale, const void* zeros, void* out, int out_ld,
                           natinf_stream_t stream);
/* The engine's other kernels on caller-supplied DEVICE buffers (tests): each entry launches the production kernel through the function the plan itself calls,
 * returns NATINF_EINVAL before anything is launched for an argument outside the contract stated here, and NATINF_ELAUNCH for a launch error.  16-bit means bf16
 * (f16 = 0) or IEEE half (f16 = 1); every pointer is required unless stated and, where it is read or written 16 bytes at a time, 16-byte aligned (said per entry); every other pointer is aligned to its element (refused otherwise).
 *
 * k_inc_stem, on the plan's grid.  images: uint8 [B][H][W][3] (input_kind NATINF_INCEPTION_U8_HWC) or fp32 [B][3][H][W] (NATINF_INCEPTION_F32_CHW);
 * out: 16-bit [B*149*149][row_width], 8-byte aligned: row (b*149 + oy)*149 + ox holds, at k = (ky*3 + kx)*3 + c, 2 r - 1 of pixel (2 oy + ky, 2 ox + kx) of the
 * image resized to 299 x 299 (bilinear, align_corners = False; uint8 inputs / 255 first), and zeros at k = 27 .. row_width - 1.  1 <= H, W <= 4096 (the limit of
 * natinf_inception_create), B >= 1 and B*149*149 < 2^31 (the limit of natinf_inception_forward), row_width 32 or 64, f16 0 or 1. */
int natinf_debug_inc_stem(const void* images, int input_kind, int B, int H, int W, int f16, int row_width, void* out, natinf_stream_t stream);
/* k_inc_pool<f16, mode, stride>: the 3 x 3 pool, mode 0 = max (padding never wins), 1 = average over the valid elements (count_include_pad = False).
 * x: 16-bit [B][H][W][x_ld], channels 0 .. C-1 read; out: 16-bit [B*Ho*Wo][out_ld], channels 0 .. C-1 written, Ho = (H + 2 pad - 3) / stride + 1 (Wo alike).
 * stride 1 or 2, pad 0 or 1, B >= 1, 1 <= H, W <= 65536, H + 2 pad >= 3 and W + 2 pad >= 3 (Ho, Wo >= 1), C >= 8, C % 8 == 0, x_ld and out_ld % 8 == 0 and >= C, x and out
 * 16-byte aligned, B * Ho * (C / 8) (one thread each) < 2^32. */
int natinf_debug_inc_pool(int f16, int mode, int stride, int pad, int B, int H, int W, int C, const void* x, int x_ld, void* out, int out_ld,
                          natinf_stream_t stream);
/* k_inc_global_avg: out[b][c] = mean over p of x[b][p][c]; x: 16-bit [B][HW][C] (no row padding), out: fp32 [B][C].  B, HW, C >= 1, B * C < 2^31. */
int natinf_debug_inc_global_avg(int f16, int B, int HW, int C, const void* x, float* out, natinf_stream_t stream);
/* The BatchNorm fold (eval, eps 1e-3) of one BasicConv2d: s[n] = gamma[n] / sqrt(var[n] + 1e-3), W'[n][(ky*kw + kx)*Cp + c] = w[n][c][ky][kx] * s[n],
 * bias[n] = beta[n] - mean[n] * s[n]; zero for c >= C, for k >= kh*kw*Cp and in rows N .. Np-1 (bias too).  w: fp32 [N][C][kh][kw]; gamma, beta, mean, var: fp32 [N];
 * bias: fp32 [Np].  f16 = 0: k_inc_pack, wp: bf16 [Np][2 Kp], columns [0, Kp) = bf16(W'), [Kp, 2 Kp) = bf16(W' - that); deq is not used (may be NULL).
 * f16 = 1: k_inc_pack_f16 on a grid of Np rows, wp: half [Np][Kp] = half(W' / deq[n]), deq: fp32 [Np], the power of two that puts the row's largest magnitude in
 * [0.5, 1) (1 for an all-zero row).  1 <= N <= Np, 1 <= C <= Cp, kh, kw >= 1, Kp >= kh*kw*Cp, Kp % 32 == 0, Np * 2 Kp < 2^31. */
int natinf_debug_inc_pack(int f16, const float* w, const float* gamma, const float* beta, const float* mean, const float* var, int N, int Np, int C, int Cp,
                          int kh, int kw, int Kp, void* wp, float* bias, float* deq, natinf_stream_t stream);
/* k_inc_im2col (plan 0, the VAE encoder's and the `ddpm` plan's stride-2 convolutions): out[(b*Ho + oy)*Wo + ox][(ky*kw + kx)*C + c] =
 * x[b][oy*stride - ph + ky][ox*stride - pw + kx][c], zero for padding taps and for k = kh*kw*C .. Kp-1; a copy of 16-bit words (either format).
 * x: [B][H][W][ld], out: [B*Ho*Wo][Kp], both 16-byte aligned; B, kh, kw, stride >= 1, 1 <= H, W <= 65536, 0 <= ph, pw <= 4096, H + 2 ph >= kh and W + 2 pw >= kw (Ho, Wo >= 1),
 * C >= 8, C % 8 == 0, ld % 8 == 0, ld >= C, Kp % 8 == 0, Kp >= kh*kw*C, B * Ho * Wo * (Kp / 8) (one thread each) < 2^31. */
int natinf_debug_inc_im2col(int B, int H, int W, int ld, int C, int kh, int kw, int stride, int ph, int pw, int Kp, const void* x, void* out,
                            natinf_stream_t stream);
int64_t natinf_inception_param_count(natinf_inception_t h);
int64_t natinf_inception_packed_bytes(natinf_inception_t h);
int64_t natinf_inception_workspace_bytes(natinf_inception_t h, int max_batch);

/* params_f32: for every BasicConv2d on the pool3 path, in torchvision registration order (Conv2d_1a_3x3, Conv2d_2a_3x3, Conv2d_2b_3x3,
 * Conv2d_3b_1x1, Conv2d_4a_3x3, Mixed_5b.{branch1x1, branch5x5_1, branch5x5_2, branch3x3dbl_1..3, branch_pool}, Mixed_5c, Mixed_5d,
 * Mixed_6a.{branch3x3, branch3x3dbl_1..3}, Mixed_6b..6e.{branch1x1, branch7x7_1..3, branch7x7dbl_1..5, branch_pool},
 * Mixed_7a.{branch3x3_1, branch3x3_2, branch7x7x3_1..4}, Mixed_7b / 7c.{branch1x1, branch3x3_1, branch3x3_2a, branch3x3_2b,
 * branch3x3dbl_1, branch3x3dbl_2, branch3x3dbl_3a, branch3x3dbl_3b, branch_pool}):
 *   conv.weight [out][in][kh][kw], bn.weight, bn.bias, bn.running_mean, bn.running_var  (AuxLogits and fc are not on the path). */
int natinf_inception_load(natinf_inception_t h, const float* params_f32, int64_t n_params, void* packed, int64_t packed_bytes,
                          natinf_stream_t stream);

/* features[b][0..2047] = pool3 activations of image b (fp32). */
int natinf_inception_forward(natinf_inception_t h, const void* images, int input_kind, float* features, int B, void* workspace,
                             int64_t workspace_bytes, natinf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NATINF_INCEPTION_H */
