/*
 * natinf.h -- C ABI of libnatinf.so, the MI355X (gfx950) Natural Inference engine.
 *
 * The reference (blairstar/NaturalDiffusion) has no FFI of its own: its hot path is
 * eager PyTorch inside three scripts.  Each entry point below replaces the Python
 * lines cited next to it; INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add to route those lines here.
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer owned by the caller (PyTorch allocator);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL =
 *     the null stream); nothing here allocates, frees, synchronises or throws;
 *   - return value: NATINF_OK (0) or a negative NATINF_E* code; natinf_strerror() names it;
 *   - "E" is the element count of one state tensor (B*C*H*W), must be a multiple of the
 *     vector width stated per call; tensors are contiguous unless a stride is given;
 *   - coefficient rows are passed as *sparse rows*: n_terms (index, value) pairs in
 *     ASCENDING index order, the order in which the reference's Python loops accumulate.
 *     Dropping a zero coefficient is bit-identical to keeping it for finite data
 *     (x*0 = +-0, acc + +-0 = acc); pass the zeros too ("dense rows") to reproduce the
 *     reference for non-finite data as well.  The arrays live in device memory.
 *   - all arithmetic is performed in the operand types and in the ORDER of the reference,
 *     one IEEE rounding per reference operation (the library is built -ffp-contract=off):
 *     results are bit-identical to the reference's CPU PyTorch path.
 */
#ifndef NATINF_H
#define NATINF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NATINF_ABI_VERSION 1

#define NATINF_OK        0
#define NATINF_EINVAL   (-1)   /* bad argument (null pointer, E not a multiple of the vector width, ...) */
#define NATINF_ELAUNCH  (-2)   /* the HIP runtime rejected the launch */
#define NATINF_ENODEV   (-3)   /* no gfx950 device / code object for this device */
#define NATINF_ESTATE   (-4)   /* handle in the wrong state */

typedef void* natinf_stream_t;              /* hipStream_t */

int         natinf_abi_version(void);
const char* natinf_strerror(int code);
/* 0 if a gfx950 device is current and the code object loads; NATINF_ENODEV otherwise. */
int         natinf_probe(void);

/* ------------------------------------------------------------------------------------------
 * CIFAR10 form: fp32 model I/O, fp64 x0 history, fp64 accumulate.
 * Replaces, for one step k of one batch,
 *   src/CIFAR10NaturalInference.py:219-230 (data_fn: score -> x0_hat in fp64),
 *   deps/score_sde_pytorch/models/utils.py:157 (score = -out/std, fp32),
 *   src/CIFAR10NaturalInference.py:233-238 (weighted_sum) and :299-304 (append, B[k,0]*noise, add).
 *
 *   s      = (-model_out) / std_f32                       (fp32)
 *   x0_k   = ((double)s * (sigma*sigma) + (double)x_k) / alpha        (fp64; hist[k] <- x0_k)
 *   acc    = sum over terms t (ascending idx[t] < k) of hist[idx[t]] * val[t], then + x0_k * c_diag
 *   x_next = (float)acc + b0_f32 * noise                  (fp32)
 *
 * hist: [n_slots][E] fp64, slot k is written, slots idx[t] are read.  E % 4 == 0.
 * c_diag = C[k][k] (the coefficient of the x0 computed in this very call; pass 0.0 for none).
 * ------------------------------------------------------------------------------------------ */
int natinf_step_f64hist(const float* x_k, const float* model_out, const float* noise,
                        double* hist, float* x_next,
                        const int32_t* idx, const double* val, int n_terms, double c_diag,
                        int k, double alpha, double sigma, float std_f32, float b0_f32,
                        int64_t E, natinf_stream_t stream);

/* The same step with an fp32 history and fp32 FMA accumulation ("fast mode": half the
 * history bytes; NOT bit-identical to the reference, error <= a few fp32 ulp per term). */
int natinf_step_f32hist(const float* x_k, const float* model_out, const float* noise,
                        float* hist, float* x_next,
                        const int32_t* idx, const float* val, int n_terms, float c_diag,
                        int k, float alpha, float sigma, float std_f32, float b0_f32,
                        int64_t E, natinf_stream_t stream);

/* The same step for a STOCHASTIC matrix, one whose noise matrix B has entries beyond column 0 (SDE Euler-Maruyama,
 * DDPM ancestral / DDIM-eta: x_{k+1} = sum_j C[k,j] x0_j + sum_j B[k,j] eps_j, eps_0 the initial noise, eps_j the noise
 * injected after step j-1).  Replaces the reference's general loop, src/ValidateNaturalInference.py:349-366 (seq_eps +
 * weighted_sum(past_eps_coeff[kk], ...)), on the CIFAR10 form's fp64 history:
 *
 *   x0_k, acc   as natinf_step_f64hist (hist[k] <- x0_k)
 *   nacc   = sum over terms t (ascending idx_b[t]) of (double)(eps_{idx_b[t]} * val_b[t])   (fp32 product, fp64 add;
 *            src/ValidateNaturalInference.py:198-204)
 *   x_next = (float)acc + (float)nacc                     (fp32)
 *
 * eps_0 is read from `noise`; eps_j, j >= 1, is NOT read from memory: it is generated in registers as
 * natinf_randn_philox_col_f32(..., seed, column = j) would return it (same Philox4x32-10 counter, same Box-Muller,
 * bit for bit).  Element e of image i (i = e / elems_per_image within the call) draws counter = (global index lo,
 * global index hi, quad (e % elems_per_image) / 4, j), key = (seed lo, seed hi); the global index is image_index[i]
 * (device int64 array) or, when image_index is NULL, first_index + i*index_stride.  An image's noise is therefore a
 * function of (seed, global index, column) only, whatever the batch split or GPU count.
 * A row whose only entry is column 0 (val_b[0] = b0_f32) gives exactly natinf_step_f64hist's x_next.
 * idx_b / val_b (fp32 values): the sparse row of B, columns <= k+1.  E % elems_per_image == 0, elems_per_image % 4 == 0
 * and elems_per_image / 4 < 2^32 (counter word 3 carries the column), otherwise NATINF_EINVAL.
 */
int natinf_step_f64hist_noise(const float* x_k, const float* model_out, const float* noise,
                              double* hist, float* x_next,
                              const int32_t* idx, const double* val, int n_terms, double c_diag,
                              const int32_t* idx_b, const float* val_b, int n_b,
                              int k, double alpha, double sigma, float std_f32,
                              uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                              int64_t elems_per_image, int64_t E, natinf_stream_t stream);

/* Inpainting on the CIFAR10 form: known pixels overwritten with the data diffused to the current noise level
 * (deps/score_sde_pytorch/controllable_generation.py:44-52, get_pc_inpainter).  The blend on its own, element e of image i:
 *
 *   out[e] = mask[e] ? fp32( fp32(known[e]*known_alpha_f32) + fp32(z[e]*known_std_f32) ) : x_in[e]
 *
 * z is what natinf_randn_philox_col_f32(..., seed, column = known_column) returns for that image and element (the same
 * generator call, bit for bit); the two products and the sum are three fp32 roundings.  known_std_f32 == 0.0f: no draw is made
 * and out = fp32(known*known_alpha_f32).  The blend is a SELECT, not the reference's x*(1-mask) + md*mask: for a 0/1 mask and
 * finite values the two agree except for the sign of a zero, and a NaN of the unknown side stays out of the known pixels.
 * `known`: device fp32.  `mask`: device uint8, one byte per element, non-zero = known, 4-byte aligned (read as one 32-bit
 * word per element quad).  known_image_stride / mask_image_stride: elems_per_image (one row per image of the call) or 0 (one
 * row shared by every image).  known_column >= 2^31: the noise columns of a matrix are at most N + 1, so the replacement
 * draws never collide with them.  x_in and out may be the same buffer.  image_index / first_index / index_stride /
 * elems_per_image as natinf_step_f64hist_noise.  NATINF_EINVAL, nothing launched: a NULL pointer, E % 4, elems_per_image not a
 * multiple of 4 dividing E or with 2^32 quads or more, a stride that is neither 0 nor elems_per_image, `mask` not 4-byte aligned,
 * known_column < 2^31.  The values of known_alpha_f32 and known_std_f32 are not inspected. */
int natinf_known_blend_f32(const float* x_in, float* out, const float* known, const uint8_t* mask,
                           int64_t known_image_stride, int64_t mask_image_stride,
                           float known_alpha_f32, float known_std_f32, uint32_t known_column,
                           uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                           int64_t elems_per_image, int64_t E, natinf_stream_t stream);

/* natinf_step_f64hist_noise with that blend applied to x_next in registers, before its one store: one launch per step, no
 * second pass over x and no noise slab.  hist[k] and the unblended x_next are operation for operation those of
 * natinf_step_f64hist_noise; x_next equals, byte for byte, natinf_step_f64hist_noise followed by natinf_known_blend_f32 with
 * the same known / mask / strides / known_* / seed / index arguments, and hist[k] equals that of natinf_step_f64hist_noise.
 * A deterministic matrix goes through as a one-term noise row (column 0, val_b[0] = fp32(B[k,0])): natinf_step_f64hist's bytes.
 * NATINF_EINVAL, nothing launched: every refusal of natinf_step_f64hist_noise and of natinf_known_blend_f32. */
int natinf_step_f64hist_inpaint(const float* x_k, const float* model_out, const float* noise,
                                double* hist, float* x_next,
                                const int32_t* idx, const double* val, int n_terms, double c_diag,
                                const int32_t* idx_b, const float* val_b, int n_b,
                                int k, double alpha, double sigma, float std_f32,
                                uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                                int64_t elems_per_image, int64_t E,
                                const float* known, const uint8_t* mask, int64_t known_image_stride, int64_t mask_image_stride,
                                float known_alpha_f32, float known_std_f32, uint32_t known_column, natinf_stream_t stream);

/* x0 correction on the CIFAR10 form: the predicted x0 of every image clipped (DDPM's clip_denoised) or dynamically thresholded (Imagen;
 * deps/dpm_solver_pytorch.py:416-425, dynamic_thresholding_fn, the reference's correcting_x0_fn="dynamic_thresholding") before the solver
 * uses it.  The correction on its own, in place on x0 [n_images][elems_per_image] fp64; for one image, x its n = elems_per_image values:
 *
 *   NATINF_X0_CLIP    : y[e] = x[e] < -c ? -c : (x[e] > c ? c : x[e])       c = max_val     (a NaN stays NaN; no division)
 *   NATINF_X0_DYNAMIC : a    = sort(|x|) ascending (NaN last)
 *                       rank = ratio * (double)(n - 1)                       one fp64 product, on the host
 *                       lo   = floor(rank), hi = ceil(rank), w = rank - lo
 *                       d    = a[hi] - a[lo]
 *                       q    = w < 0.5 ? fma(w, d, a[lo]) : fma(w - 1.0, d, a[hi])       ONE fused multiply-add, fp64
 *                       s    = any NaN in x ? NaN : max(q, max_val)          (a NaN q, from a[lo] = a[hi] = inf, gives s = NaN)
 *                       y[e] = s is NaN ? NaN : min(max(x[e], -s), s) / s    IEEE fp64 division
 *
 * This is torch.quantile(|x0|, ratio, dim=1), torch.maximum and torch.clamp(...) / s of the reference lines, on fp64, as ATen's CPU
 * kernels evaluate them (the interpolation inside torch.quantile is a fused multiply-add: the library's only one outside a division).  The
 * two order statistics are exact: selected on the 64-bit patterns of |x| with integer counts, so the result does not depend on the order in
 * which threads arrive.  A NaN the correction produces is the quiet NaN 0x7FF8000000000000; a NaN that CLIP passes through keeps its bits.
 * s_out: NULL or [n_images] fp64, the threshold used (CLIP: max_val).  One workgroup per image; the image lives in LDS, so
 * elems_per_image <= 8192.  NATINF_EINVAL, nothing launched: x0 NULL, n_images <= 0, elems_per_image not a positive multiple of 4 or
 * > 8192, mode neither value, ratio outside [0, 1] or NaN, max_val not finite or <= 0 (ratio is checked in CLIP mode too). */
#define NATINF_X0_CLIP    1
#define NATINF_X0_DYNAMIC 2
int natinf_x0_threshold_f64(double* x0, double* s_out, int64_t n_images, int64_t elems_per_image,
                            int mode, double ratio, double max_val, natinf_stream_t stream);

/* natinf_step_f64hist_noise with that correction between the denoiser and the history, in one launch and without a workspace: one
 * workgroup per image computes the image's raw x0 into LDS (it is never written to memory), finds the threshold, and then, per element,
 *
 *   hist[k] <- y                 byte for byte natinf_x0_threshold_f64 applied to the hist[k] natinf_step_f64hist_noise writes
 *   acc     = sum over terms t of hist[idx[t]] * val[t], then + y * c_diag      (the diagonal term uses the corrected value)
 *   x_next  = (float)acc + (float)nacc, then the blend of natinf_known_blend_f32 if known / mask are given
 *
 * everything else operation for operation natinf_step_f64hist_noise's.  `known` and `mask` may both be NULL (no blend; the strides and
 * known_* are then not inspected); with both given they are natinf_step_f64hist_inpaint's.  s_out as above.  A deterministic matrix goes
 * through as a one-term noise row (column 0, val_b[0] = fp32(B[k,0])).  "Matrix X plus this correction" is the classical solver X with
 * correcting_x0_fn: every sampler the matrices express is linear in the x0_j.
 * NATINF_EINVAL, nothing launched: every refusal of natinf_step_f64hist_inpaint (the blend's only when known / mask are given), exactly
 * one of known / mask NULL, and every refusal of natinf_x0_threshold_f64 for mode / ratio / max_val / elems_per_image.  All of them are
 * pure argument checks: a refusal touches no device (like natinf_step_f64hist_noise, the entry does not read idx_b back). */
int natinf_step_f64hist_x0fix(const float* x_k, const float* model_out, const float* noise,
                              double* hist, float* x_next,
                              const int32_t* idx, const double* val, int n_terms, double c_diag,
                              const int32_t* idx_b, const float* val_b, int n_b,
                              int k, double alpha, double sigma, float std_f32,
                              uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                              int64_t elems_per_image, int64_t E,
                              const float* known, const uint8_t* mask, int64_t known_image_stride, int64_t mask_image_stride,
                              float known_alpha_f32, float known_std_f32, uint32_t known_column,
                              int mode, double ratio, double max_val, double* s_out, natinf_stream_t stream);

/* Super-resolution on the CIFAR10 form: the predicted x0 of every image projected onto the pictures whose s x s block averages are a given
 * low-resolution picture, x0 <- x0 + A+(low - A x0) with A the block average and A+ pixel replication (the range-null-space correction of DDNM,
 * Wang et al. 2022).  The projection on its own, in place on x0 [n_images][elems_per_image] fp64.  An image is `channels` planes of
 * height x width values in NCHW order, elems_per_image = channels*height*width; scale = s in {2, 4, 8}.  For block (c, I, J), x[c][r][w] the
 * image's values and low[c][I][J] the given low-resolution value (fp64, [channels][height/s][width/s]):
 *
 *   r_j  = x[c][sI+j][sJ] + x[c][sI+j][sJ+1] + ... + x[c][sI+j][sJ+s-1]     left to right, plain fp64 adds, started from the first element
 *   S    = r_0 + r_1 + ... + r_{s-1}                                          top to bottom, likewise (no zero seed in either sum)
 *   m    = S * 2^(-2 log2 s)                                                  one fp64 multiply (exact unless it underflows)
 *   d    = low[c][I][J] - m
 *   y[e] = x[e] + d          for every element e of the block; a NaN result is stored as 0x7FF8000000000000
 *   r    = max over the image's blocks of |d|, compared as the 64-bit patterns of |d| (a NaN pattern sorts above +inf); a NaN maximum is that
 *          same quiet NaN
 *
 * No operation is fused.  The row-then-column order is part of the definition (a thread may own a block row without changing a bit), and r is
 * an integer maximum, so nothing depends on the order in which threads arrive: no float atomics, no global atomics, no workspace.
 * r_out: NULL or [n_images] fp64, how far the image's block means were from the data.  low_image_stride: elems_per_image / s^2 (one picture per
 * image of the call) or 0 (one picture for every image).  One workgroup per image; the image lives in LDS, so elems_per_image <= 8192.  `width`
 * need not be a multiple of 4: an element quad may straddle rows and blocks.
 * NATINF_EINVAL, nothing launched: x0 or low NULL, n_images <= 0, scale not 2, 4 or 8, channels, height or width <= 0, height or width not a
 * multiple of scale, channels*height*width not a multiple of 4 or > 8192, low_image_stride neither 0 nor channels*height*width / s^2. */
int natinf_x0_project_f64(double* x0, const double* low, double* r_out, int64_t n_images, int channels, int height, int width, int scale,
                          int64_t low_image_stride, natinf_stream_t stream);

/* natinf_step_f64hist_noise with that projection between the denoiser and the history, in one launch and without a workspace: one workgroup
 * per image computes the image's raw x0 into LDS (it is never written to memory), finds the block residuals d, and then, per element,
 *
 *   hist[k] <- y                 byte for byte natinf_x0_project_f64 applied to the hist[k] natinf_step_f64hist_noise writes
 *   acc     = sum over terms t of hist[idx[t]] * val[t], then + y * c_diag      (the diagonal term uses the projected value)
 *   x_next  = (float)acc + (float)nacc
 *
 * everything else operation for operation natinf_step_f64hist_noise's.  Every sampler the matrices express is linear in the x0_j, so "matrix X
 * plus this projection" is the classical solver X run as DDNM, and every history row satisfies A x0_j = low up to rounding.  A deterministic
 * matrix goes through as a one-term noise row (column 0, val_b[0] = fp32(B[k,0])).  There are no known pixels here: the projection is not
 * composed with the inpainting, colorization or correction entries.  r_out as above.
 * NATINF_EINVAL, nothing launched: every refusal of natinf_step_f64hist_noise for its own arguments, and every refusal of
 * natinf_x0_project_f64 for low / channels / height / width / scale / low_image_stride, with channels*height*width != elems_per_image
 * refused too.  All of them are pure argument checks: a refusal touches no device. */
int natinf_step_f64hist_project(const float* x_k, const float* model_out, const float* noise,
                                double* hist, float* x_next,
                                const int32_t* idx, const double* val, int n_terms, double c_diag,
                                const int32_t* idx_b, const float* val_b, int n_b,
                                int k, double alpha, double sigma, float std_f32,
                                uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                                int64_t elems_per_image, int64_t E,
                                const double* low, int64_t low_image_stride, int channels, int height, int width, int scale,
                                double* r_out, natinf_stream_t stream);

/* Colorization on the CIFAR10 form: the gray channel of a rotated colour space overwritten with the gray data diffused to the
 * current noise level (deps/score_sde_pytorch/controllable_generation.py:85-181, get_pc_colorizer; :142 with mask = (1, 0, 0)).
 * An image is three planes of P = elems_per_image / 3 elements (NCHW).  The blend on its own, pixel p of image i, with
 * x = (x0, x1, x2) the values of planes 0, 1, 2 at p, M = basis and W = inverse (row-major, M[r][c] = basis[3*r + c]):
 *
 *   dot3(a,b,c; p,q,r) = fp32( fp32( fp32(a*p) + fp32(b*q) ) + fp32(c*r) )
 *   u1    = dot3(x0,x1,x2; M[0][1],M[1][1],M[2][1])
 *   u2    = dot3(x0,x1,x2; M[0][2],M[1][2],M[2][2])
 *   u0    = gray_std_f32 != 0 ? fp32( fp32(gray_u[p]*gray_alpha_f32) + fp32(z[p]*gray_std_f32) ) : fp32(gray_u[p]*gray_alpha_f32)
 *   out_c = dot3(u0,u1,u2; W[0][c],W[1][c],W[2][c])        c = 0, 1, 2
 *
 * No product and sum is ever fused.  The old latent channel 0 is fully replaced, so it is never computed.  z is what
 * natinf_randn_philox_col_f32(..., seed, column = gray_column) returns for PLANE 0 of that image (the same generator call, bit
 * for bit: the element quad of plane 0 is the pixel quad); gray_std_f32 == 0.0f: no draw is made.  Unlike the inpainting select,
 * a NaN in x reaches all three outputs of its pixel: that is the rotation.
 * `gray_u`: device fp32, one value per pixel: latent channel 0 of the known picture, dot3(k0,k1,k2; M[0][0],M[1][0],M[2][0]),
 * prepared by the caller; read as one 16-byte load per pixel quad.  gray_image_stride: elems_per_image / 3 (one row per image of
 * the call) or 0 (one picture shared by every image).  `basis`, `inverse`: HOST arrays of 9 floats, read at call time and carried
 * to the kernel by value; the library hard-codes neither (any orthonormal basis and its inverse will do).
 * Columns: a matrix's noise columns are 0..N+1, the inpainting draws 2^31 + level, the colorization draws 2^31 + 2^30 + level:
 * the three families are disjoint for N < 2^30.  The AutoencoderKL posterior draw (natinf_vae.h) uses the one column 0xE0000000
 * = 2^31 + 2^30 + 2^29: outside all three for level < 2^29.  x_in and out may be the same buffer.  image_index / first_index / index_stride
 * / elems_per_image as natinf_step_f64hist_noise.  NATINF_EINVAL, nothing launched: a NULL x_in, out, gray_u, basis or inverse,
 * E % 4, elems_per_image not a multiple of 4 dividing E or with 2^32 quads or more, elems_per_image % 12 != 0 (three planes of
 * whole quads), a gray_image_stride that is neither 0 nor elems_per_image / 3, gray_column < 0xC0000000.  The values of
 * gray_alpha_f32, gray_std_f32 and the matrices are not inspected. */
int natinf_color_blend_f32(const float* x_in, float* out, const float* gray_u, int64_t gray_image_stride,
                           const float basis[9], const float inverse[9],
                           float gray_alpha_f32, float gray_std_f32, uint32_t gray_column,
                           uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                           int64_t elems_per_image, int64_t E, natinf_stream_t stream);

/* natinf_step_f64hist_noise with that blend applied to x_next in registers: one launch per step, one thread per pixel quad, which
 * runs natinf_step_f64hist_noise's arithmetic on the element quad of each plane in turn, blends the three results and stores them.
 * hist[k] and the unblended x_next are operation for operation those of natinf_step_f64hist_noise; x_next equals, byte for byte,
 * natinf_step_f64hist_noise followed by natinf_color_blend_f32 with the same gray_* / basis / inverse / seed / index arguments, and
 * hist[k] equals that of natinf_step_f64hist_noise.  A deterministic matrix goes through as a one-term noise row (column 0,
 * val_b[0] = fp32(B[k,0])).  NATINF_EINVAL, nothing launched: every refusal of natinf_step_f64hist_noise and of
 * natinf_color_blend_f32. */
int natinf_step_f64hist_colorize(const float* x_k, const float* model_out, const float* noise,
                                 double* hist, float* x_next,
                                 const int32_t* idx, const double* val, int n_terms, double c_diag,
                                 const int32_t* idx_b, const float* val_b, int n_b,
                                 int k, double alpha, double sigma, float std_f32,
                                 uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                                 int64_t elems_per_image, int64_t E,
                                 const float* gray_u, int64_t gray_image_stride, const float basis[9], const float inverse[9],
                                 float gray_alpha_f32, float gray_std_f32, uint32_t gray_column, natinf_stream_t stream);

/* src/CIFAR10NaturalInference.py:233-238 on its own: out = (float) sum_t hist[idx[t]]*val[t]. */
int natinf_weighted_sum_f64(const double* hist, float* out,
                            const int32_t* idx, const double* val, int n_terms,
                            int64_t E, natinf_stream_t stream);

/* Initial noise for batch-sharded generation (replaces the sequential torch.manual_seed(888) + torch.randn of
 * src/CIFAR10NaturalInference.py:285-290, which cannot be split over GPUs): out[i][e], i < n_images, e <
 * elems_per_image, ~ N(0,1) from Philox4x32-10 with key = seed and counter = (global image index, e/4), Box-Muller.
 * The global index of row i is image_index[i] (device array) or, when image_index is NULL, first_index +
 * i*index_stride.  The same (seed, global index) gives the same image for any GPU count or batch split.
 * elems_per_image % 4 == 0. */
int natinf_randn_philox_f32(float* out, int64_t n_images, int64_t elems_per_image, const int64_t* image_index,
                            int64_t first_index, int64_t index_stride, uint64_t seed, natinf_stream_t stream);

/* natinf_randn_philox_f32 for noise column `column` of a stochastic matrix: counter = (global image index lo, hi,
 * e/4, column).  Column 0 is natinf_randn_philox_f32 itself (word 3 = (e/4) >> 32), bit for bit; for column > 0 the
 * quad must fit word 2 (elems_per_image / 4 < 2^32, else NATINF_EINVAL).  These are exactly the eps_j that
 * natinf_step_f64hist_noise injects. */
int natinf_randn_philox_col_f32(float* out, int64_t n_images, int64_t elems_per_image, const int64_t* image_index,
                                int64_t first_index, int64_t index_stride, uint64_t seed, uint32_t column,
                                natinf_stream_t stream);

/* src/CIFAR10NaturalInference.py:212-216 (to_pixel): x [B,C,H,W] fp32 -> uint8 [B,H,W,C] =
 * trunc(clip(x*255, 0, 255)); with centered != 0 the inverse scaler of datasets.py:32-38,
 * x <- (x+1)/2, is applied first (the reference calls the two back to back, :308-309). */
int natinf_to_pixel_u8(const float* x, uint8_t* out, int B, int C, int H, int W, int centered,
                       natinf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Validate (DiT, eps-prediction) form: fp32 tensors, fp32 products accumulated in fp64.
 * Replaces src/ValidateNaturalInference.py:193 (CFG fuse), :355 (pred_x0), :198-204 x2
 * (weighted_sum over x0 and over eps histories) and :362-366.
 *
 *   eps    = uncond ? uncond + cfg*(cond - uncond) : cond                 (fp32, three roundings)
 *   x0_k   = c1_f32*z - c2_f32*eps                                        (fp32; hist_x0[k] <- x0_k)
 *   a      = sum_t (double)(hist_x0[idx_c[t]] * val_c[t])  [+ (double)(x0_k*c_diag)]   (fp64 adds)
 *   b      = sum_t (double)(hist_eps[idx_b[t]] * val_b[t])                              (fp64 adds)
 *   z_next = (float)a + (float)b
 *
 * cond/uncond may be strided views of a [B, 2*C, H, W] DiT output (learn_sigma): element e of
 * sample n sits at n*eps_sample_stride + (e % sample_elems).  hist_eps [n_slots+1][E] already
 * holds every noise the row refers to (slot 0 = initial noise, slot j = the draw after step j-1).
 * E % 4 == 0, sample_elems % 4 == 0.
 *
 * Four entries share this arithmetic: natinf_step_f32prod (noises read from the hist_eps slab), natinf_step_f32prod_noise
 * (noises drawn in the kernel; one cfg and uncond row i for image i), natinf_step_f32prod_noise_guided (the same with
 * a scale and an unconditional row PER IMAGE: guidance intervals and mixed-scale batches) and natinf_step_f32prod_inpaint
 * (the per-image form with the known latents blended into z_next before its store: latent-space inpainting).
 * ------------------------------------------------------------------------------------------ */
int natinf_step_f32prod(const float* z, const float* cond, const float* uncond, float cfg,
                        int64_t sample_elems, int64_t eps_sample_stride,
                        float* hist_x0, const float* hist_eps, float* z_next,
                        const int32_t* idx_c, const float* val_c, int n_c, float c_diag,
                        const int32_t* idx_b, const float* val_b, int n_b,
                        int k, float c1_f32, float c2_f32,
                        int64_t E, natinf_stream_t stream);

/* The same step with the noise row generated in registers (a generation job: no hist_eps slab, noise keyed by the global
 * image index).  eps, x0_k, a and z_next operation for operation as natinf_step_f32prod; only the source of eps_j in
 *
 *   b      = sum over terms t (ascending idx_b[t]) of (double)(eps_{idx_b[t]} * val_b[t])
 *
 * differs: eps_0 is read from `noise` ([E] fp32, the initial noise); eps_j, j >= 1, is NOT read from memory: it is
 * generated as natinf_randn_philox_col_f32(..., seed, column = j) would return it (same Philox4x32-10 counter, same
 * Box-Muller, bit for bit).  An image is one sample of sample_elems elements; element e of image i = e / sample_elems
 * draws counter = (global index lo, global index hi, quad (e % sample_elems) / 4, j), key = (seed lo, seed hi); the
 * global index is image_index[i] (device int64 array) or, when image_index is NULL, first_index + i*index_stride.
 * So z_next and hist_x0[k] equal, byte for byte, natinf_step_f32prod on a hist_eps slab whose row 0 is `noise` and whose
 * row j >= 1 natinf_randn_philox_col_f32(column = j) filled, and an image's trajectory is a function of (seed, global
 * index) whatever the batch split or GPU count.  A deterministic matrix (column 0 only) goes through unchanged.
 * n_b == 0 is legal (b = 0).  NATINF_EINVAL, nothing launched: E % 4, sample_elems % 4, E % sample_elems,
 * sample_elems / 4 >= 2^32 (counter word 3 carries the column), n_b > k + 2 or an idx_b entry outside 0..k+1 (eps_j is
 * drawn after step j-1), `noise` NULL when the row names column 0.  For that check the n_b indices are read back from the
 * device on a private stream before the launch: the host waits for that copy alone, not for `stream`; idx_b must be
 * complete when the call is made (a row table uploaded once), and the call cannot be part of a stream capture. */
int natinf_step_f32prod_noise(const float* z, const float* cond, const float* uncond, float cfg,
                              int64_t sample_elems, int64_t eps_sample_stride,
                              float* hist_x0, const float* noise, float* z_next,
                              const int32_t* idx_c, const float* val_c, int n_c, float c_diag,
                              const int32_t* idx_b, const float* val_b, int n_b,
                              int k, float c1_f32, float c2_f32,
                              uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                              int64_t E, natinf_stream_t stream);

/* natinf_step_f32prod_noise with per-image guidance (a guidance interval, a scale sweep, guided and unguided images in
 * one batch): every image carries its own CFG scale, and the unconditional rows are compacted to the images that are
 * guided.  With n_images = E / sample_elems, the model's eps of image i is
 *
 *   uncond_slot[i] < 0 : eps = cond[i]
 *   otherwise          : u = uncond[uncond_slot[i]] ; d = cond[i] - u ; m = cfg_image[i]*d ; eps = u + m
 *
 * (fp32, the three roundings of the launch-wide form in the same order); x0_k, a, b and z_next are those of
 * natinf_step_f32prod_noise.  cfg_image: device [n_images] fp32.  uncond_slot: device [n_images] int32, each -1 or a row
 * 0..n_uncond-1 of `uncond`; rows may repeat or be left out.  `uncond` holds n_uncond samples at the per-sample stride of
 * `cond` (eps_sample_stride), so it may be the tail of a denoiser output [n_images + n_uncond, 2*C, H, W]; it may be
 * NULL when n_uncond == 0.  cfg_image[i] of an image without a slot is not read.
 *
 * Identity rule: with cfg_image[i] == cfg and uncond_slot[i] == i for every i, z_next and hist_x0[k] are byte for byte
 * those of natinf_step_f32prod_noise(..., uncond, cfg, ...); with every slot -1 they are those of that entry with
 * uncond == NULL.  A step is a per-image function, so a mixed launch gives each image the bytes of that entry run on the
 * images that share its scale.
 *
 * NATINF_EINVAL, nothing launched: every refusal of natinf_step_f32prod_noise; cfg_image or uncond_slot NULL;
 * n_uncond < 0; n_uncond > 0 with `uncond` NULL; a slot outside -1..n_uncond-1.  The slots are checked the way idx_b
 * is: read back on the same private stream before the launch, so uncond_slot must be complete when the call is made (a
 * table uploaded once per batch) and the call cannot be part of a stream capture.  The VALUES of cfg_image are not
 * inspected (any fp32, NaN included, goes into the arithmetic above), and it is read by the kernel only, in stream order. */
int natinf_step_f32prod_noise_guided(const float* z, const float* cond, const float* uncond,
                                     const float* cfg_image, const int32_t* uncond_slot, int n_uncond,
                                     int64_t sample_elems, int64_t eps_sample_stride,
                                     float* hist_x0, const float* noise, float* z_next,
                                     const int32_t* idx_c, const float* val_c, int n_c, float c_diag,
                                     const int32_t* idx_b, const float* val_b, int n_b,
                                     int k, float c1_f32, float c2_f32,
                                     uint64_t seed, const int64_t* image_index, int64_t first_index, int64_t index_stride,
                                     int64_t E, natinf_stream_t stream);

/* natinf_step_f32prod_noise_guided with the blend of natinf_known_blend_f32 applied to z_next in registers, before its one
 * store: latent-space inpainting in one launch per step, no second pass over z and no noise slab.  An image of the blend is one
 * sample (elems_per_image = sample_elems), and the blend shares the step's seed and global image indices:
 *
 *   z_next[e] = mask[e] ? fp32( fp32(known[e]*known_alpha_f32) + fp32(n[e]*known_std_f32) ) : (float)a + (float)b
 *
 * n = what natinf_randn_philox_col_f32(..., seed, column = known_column) returns for that image and element; known_std_f32 ==
 * 0.0f draws nothing.  `known` (device fp32), `mask` (device uint8, ONE BYTE PER LATENT ELEMENT, non-zero = known, 4-byte
 * aligned: a per-pixel mask is broadcast over the channels by the caller), the two strides (sample_elems, or 0 for one row
 * shared by every image) and known_column (>= 2^31) are natinf_known_blend_f32's.
 *
 * Contract: z_next equals, byte for byte, natinf_step_f32prod_noise_guided followed by natinf_known_blend_f32 with the same
 * known / mask / strides / known_* / seed / index arguments and elems_per_image = sample_elems; hist_x0[k] is that of
 * natinf_step_f32prod_noise_guided (the unblended entry's: the history never sees the blend).  Through that entry's identity
 * rule, cfg_image[i] == cfg with uncond_slot[i] == i gives the bytes of natinf_step_f32prod_noise + blend, every slot -1 those
 * of natinf_step_f32prod_noise with uncond == NULL + blend.  A select, so a NaN of the unblended side stays out of the known
 * elements.
 *
 * NATINF_EINVAL, nothing launched: every refusal of natinf_step_f32prod_noise_guided, and every refusal of
 * natinf_known_blend_f32 with elems_per_image = sample_elems (known or mask NULL, a stride that is neither 0 nor
 * sample_elems, `mask` not 4-byte aligned, known_column < 2^31).  All the pure argument checks, the blend's included, are made
 * before idx_b and uncond_slot are read back, so such a refusal touches no device.  The read-backs are those of the guided
 * entry (same private stream, same rules for captures). */
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
                                float known_alpha_f32, float known_std_f32, uint32_t known_column, natinf_stream_t stream);

/* src/ValidateNaturalInference.py:198-204 on its own. */
int natinf_weighted_sum_f32prod(const float* hist, float* out,
                                const int32_t* idx, const float* val, int n_terms,
                                int64_t E, natinf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SD3 (flow, all-fp16 chain) form.  Replaces src/SD3NaturalInference.py:157-168 (row-normalised
 * weighted mean), :209 (next model input), :215-219 (x0 from velocity, CFG fuse, append); with
 * NATINF_SD3_CFG_ON_VELOCITY it is the Euler twin, :61-69 and :117-129.
 *
 *   default:  x0n = x - sig*v_null ; x0t = x - sig*v_text ; f = x0n + cfg*(x0t - x0n)
 *   velocity: v = v_null + cfg*(v_text - v_null) ; f = x - sig*v
 *   hist[k] <- f
 *   acc    = fp16 chain over terms t (ascending idx[t] < k) of hist[idx[t]]*val[t], then f*c_diag
 *   mean   = acc / w_total                                   (-> mean_out, may be NULL)
 *   x_next = sig_next*noise + one_minus_sig_next*mean        (-> x_next, may be NULL on the last step)
 *
 * Every product / sum / quotient is formed in fp32 from fp16 operands and rounded to fp16, as
 * eager PyTorch does; scalars are fp32 (`sig`, `sig_next`, `one_minus_sig_next` must already hold
 * the fp16-rounded value of the 0-d tensor the reference multiplies with).  E % 8 == 0.
 *
 * Three entries share this arithmetic: natinf_step_f16chain (one cfg, v_null image i for image i),
 * natinf_step_f16chain_guided (a scale and a null-prompt row PER IMAGE: guidance intervals and mixed-scale batches) and
 * natinf_step_f16chain_inpaint (the per-image form with the known latents blended into x_next before its store).
 * ------------------------------------------------------------------------------------------ */
#define NATINF_SD3_CFG_ON_VELOCITY 1
int natinf_step_f16chain(const void* x, const void* v_text, const void* v_null, const void* noise,
                         void* hist, void* mean_out, void* x_next,
                         const int32_t* idx, const float* val, int n_terms, float c_diag, float w_total,
                         int k, float sig, float sig_next, float one_minus_sig_next, float cfg,
                         int flags, int64_t E, natinf_stream_t stream);

/* natinf_step_f16chain with per-image guidance (a guidance interval, a scale sweep, guided and unguided images in one
 * batch): every image carries its own CFG scale, and the null-prompt velocities are compacted to the images that are
 * guided.  An image is sample_elems consecutive elements; with n_images = E / sample_elems, the fused x0 of image i is
 *
 *   uncond_slot[i] < 0 : f = x - sig*v_text                                   (either flag value)
 *   otherwise          : u = v_null[uncond_slot[i]] ; cfg = cfg_image[i] ;
 *                        default:  x0n = x - sig*u ; x0t = x - sig*v_text ; f = x0n + cfg*(x0t - x0n)
 *                        velocity: v = u + cfg*(v_text - u) ; f = x - sig*v
 *
 * (every operation rounded to fp16, the roundings of the launch-wide form in the same order); hist[k], acc, mean and
 * x_next are those of natinf_step_f16chain.  cfg_image: device [n_images] fp32.  uncond_slot: device [n_images] int32,
 * each -1 or a row 0..n_uncond-1 of `v_null`; rows may repeat or be left out.  `v_null` holds n_uncond images of
 * sample_elems fp16 elements, contiguous, so it may be the tail of a transformer output [n_images + n_uncond, C, H, W]; it
 * may be NULL when n_uncond == 0.  `x` and `v_text` hold all n_images.  Neither cfg_image[i] nor any element of v_null is
 * read for an image without a slot.
 *
 * Identity rule: with cfg_image[i] == cfg and uncond_slot[i] == i for every i, hist[k], mean_out and x_next are byte for
 * byte those of natinf_step_f16chain(..., v_null, ..., cfg, flags, ...).  A step is a per-image function, so a mixed launch
 * gives each image the bytes of that entry run on the images that share its scale.
 *
 * NATINF_EINVAL, nothing launched: every refusal of natinf_step_f16chain (except that v_null may be NULL when
 * n_uncond == 0); cfg_image or uncond_slot NULL; n_uncond < 0; n_uncond > 0 with `v_null` NULL; sample_elems not a
 * positive multiple of 8 dividing E; a slot outside -1..n_uncond-1.  The slots are checked the way
 * natinf_step_f32prod_noise_guided checks them: read back on the same private stream before the launch, so uncond_slot
 * must be complete when the call is made (a table uploaded once per batch) and the call cannot be part of a stream
 * capture.  The VALUES of cfg_image are not inspected (any fp32, NaN included, goes into the arithmetic above), and it
 * is read by the kernel only, in stream order. */
int natinf_step_f16chain_guided(const void* x, const void* v_text, const void* v_null,
                                const float* cfg_image, const int32_t* uncond_slot, int n_uncond, int64_t sample_elems,
                                const void* noise, void* hist, void* mean_out, void* x_next,
                                const int32_t* idx, const float* val, int n_terms, float c_diag, float w_total,
                                int k, float sig, float sig_next, float one_minus_sig_next,
                                int flags, int64_t E, natinf_stream_t stream);

/* Latent-space inpainting on the SD3 form: the known latents at the flow level (sig, one_minus_sig), blended into x.
 *
 *   out[e] = mask[e] ? fp16( fp16(sig*n[e]) + fp16(one_minus_sig*known[e]) ) : x_in[e]
 *
 * the known side is natinf_flow_input_f16 with mean = known, in its order of fp16 roundings; sig and one_minus_sig already hold
 * fp16-rounded values, as for natinf_step_f16chain.  A select: a NaN of x_in stays out of the known elements.  x_in, out, noise and
 * known are fp16; out may be x_in.  `mask`: device uint8, ONE BYTE PER LATENT ELEMENT, non-zero = known, 8-byte aligned (one
 * 64-bit word per 8 elements; a per-cell mask is broadcast over the channels by the caller).  known_image_stride /
 * mask_image_stride: elems_per_image (one row per image) or 0 (one row shared by every image).  The noise side n is chosen by
 * known_column:
 *
 *   0        ("same"):  n = noise[e], the image's own initial noise ([E] fp16; must not be NULL)
 *   >= 2^31  ("fresh"): n = what natinf_randn_philox_col_f32(..., seed, column = known_column) returns for that image and element,
 *                       rounded to fp16 once; `noise` is not read and may be NULL.  Element e of image i = e / elems_per_image draws
 *                       counter = (global index lo, global index hi, quad (e % elems_per_image) / 4, known_column); the global index
 *                       is image_index[i] or, when image_index is NULL, first_index + i*index_stride.
 *
 * An 8-vector whose mask word is 0 draws nothing and does not read `known`.  NATINF_EINVAL, nothing launched: x_in, out, known or
 * mask NULL; E % 8; elems_per_image not a positive multiple of 8 dividing E, or elems_per_image / 4 >= 2^32; a stride that is
 * neither 0 nor elems_per_image; `mask` not 8-byte aligned; known_column in 1..2^31-1; known_column == 0 with `noise` NULL. */
int natinf_known_blend_f16(const void* x_in, void* out, const void* noise, const void* known, const uint8_t* mask,
                           int64_t known_image_stride, int64_t mask_image_stride,
                           float sig, float one_minus_sig, uint32_t known_column, uint64_t seed,
                           const int64_t* image_index, int64_t first_index, int64_t index_stride,
                           int64_t elems_per_image, int64_t E, natinf_stream_t stream);

/* natinf_step_f16chain_guided with the blend of natinf_known_blend_f16 applied to x_next in registers, before its one store:
 * latent-space inpainting in one launch per step, no second pass over x.  An image of the blend is sample_elems elements, and the
 * blend's level is the step's own (sig_next, one_minus_sig_next):
 *
 *   x_next[e]   = mask[e] ? fp16( fp16(sig_next*n[e]) + fp16(one_minus_sig_next*known[e]) ) : sig_next*noise + one_minus_sig_next*mean
 *   mean_out[e] = (flags & NATINF_SD3_BLEND_MEAN) && mask[e] ? known[e] : mean[e]
 *
 * n, known, mask, the two strides, known_column, seed and the index arguments are natinf_known_blend_f16's; in "same" mode n is
 * the `noise` the flow input reads.  NATINF_SD3_BLEND_MEAN is for the last step of a job, whose result is the mean: the known
 * elements of the result are then `known` itself.  Both values of NATINF_SD3_CFG_ON_VELOCITY are taken.
 *
 * Contract: hist[k] is that of natinf_step_f16chain_guided (the history never sees the blend); x_next equals, byte for byte, that
 * entry followed by natinf_known_blend_f16(x_next, x_next, noise, known, mask, strides, sig_next, one_minus_sig_next, known_column,
 * seed, index arguments, elems_per_image = sample_elems); without NATINF_SD3_BLEND_MEAN mean_out is that entry's.  Through its
 * identity rule, cfg_image[i] == cfg with uncond_slot[i] == i gives the bytes of natinf_step_f16chain on the unknown side.
 *
 * NATINF_EINVAL, nothing launched: every refusal of natinf_step_f16chain_guided (NATINF_SD3_BLEND_MEAN is accepted here and
 * nowhere else) and every refusal of natinf_known_blend_f16 with elems_per_image = sample_elems (known_column == 0 needs `noise`
 * only when x_next is given).  All the pure argument checks, the blend's included, are made before uncond_slot is read back, so
 * such a refusal touches no device.  The read-back is that of the guided entry (same private stream, same rules for captures). */
#define NATINF_SD3_BLEND_MEAN 2
int natinf_step_f16chain_inpaint(const void* x, const void* v_text, const void* v_null,
                                 const float* cfg_image, const int32_t* uncond_slot, int n_uncond, int64_t sample_elems,
                                 const void* noise, void* hist, void* mean_out, void* x_next,
                                 const int32_t* idx, const float* val, int n_terms, float c_diag, float w_total,
                                 int k, float sig, float sig_next, float one_minus_sig_next,
                                 int flags, int64_t E,
                                 const void* known, const uint8_t* mask, int64_t known_image_stride, int64_t mask_image_stride,
                                 uint32_t known_column, uint64_t seed,
                                 const int64_t* image_index, int64_t first_index, int64_t index_stride, natinf_stream_t stream);

/* src/SD3NaturalInference.py:209 on its own: out = sig*noise + one_minus_sig*mean (fp16 ops; mean may be
 * NULL = zeros, the k = 0 case of :207). */
int natinf_flow_input_f16(const void* noise, const void* mean, void* out, float sig, float one_minus_sig,
                          int64_t E, natinf_stream_t stream);

/* src/SD3NaturalInference.py:157-168 on its own (fp16 in, fp16 out). */
int natinf_weighted_mean_f16(const void* hist, void* out,
                             const int32_t* idx, const float* val, int n_terms, float w_total,
                             int64_t E, natinf_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * NCSN++ / DDPM++ denoiser (CIFAR10 VP continuous) -- replaces the `model(x, labels)` call of
 * deps/score_sde_pytorch/models/utils.py:144-160, i.e. NCSNpp.forward
 * (deps/score_sde_pytorch/models/ncsnpp.py:232-381) under
 * configs/vp/cifar10_ddpmpp_continuous.py:41-64.  Declared in natinf_ncsnpp.h.
 * ------------------------------------------------------------------------------------------ */

#ifdef __cplusplus
}
#endif
#endif /* NATINF_H */
