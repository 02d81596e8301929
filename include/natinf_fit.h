/*
 * natinf_fit.h -- C ABI of the coefficient fitter's hot path inside libnatinf.so: one fp64 Gram matrix per image over rows of the fp64 x0 history
 * (natinf_step_f64hist's slab), the image's initial noise and a target state.  Every quantity of the row-wise least-squares problem "which
 * combination of the student's own x0 predictions lands closest to the teacher's state" is an entry of it (naturaldiffusion_amd/fit.py; DESIGN.md
 * section 4d-fit).  The Gram matrices of such histories reach condition numbers of 1e12, hence fp64 inputs and fp64 accumulation throughout.
 *
 * Definition.  For image i of the call, M = n_rows + 2 vectors of elems_per_image (epi) values:
 *
 *   v_t        = hist[rows[t] * hist_stride + i * epi .. + epi)      t < n_rows       fp64
 *   v_{n_rows}   = noise [i * epi .. + epi)                                           fp32, widened exactly
 *   v_{n_rows+1} = target[i * epi .. + epi)                                           fp32, widened exactly
 *   gram[i][a][b] = sum_e v_a[e] * v_b[e]                                             fp64
 *
 * The caller offsets hist, noise and target to the first image of the call, so a [slot][E] history slab is read in place for any sub-range of a
 * batch: hist_stride is the slab's E.  History slots that rows does not name are never read.
 *
 * Summation order (fixed; no floating-point atomics).  One workgroup of NATINF_FIT_WAVES waves of 64 lanes forms gram[i].  The elements go in steps of 16:
 * step s = elements 16 s .. 16 s + 15 belongs to wave s mod NATINF_FIT_WAVES, and a wave takes its steps in ascending order.  A step is four issues
 * j = 0 .. 3 of v_mfma_f64_16x16x4_f64 into the wave's running accumulator; issue j adds the four products at elements 16 s + 4 q + j, q = 0 .. 3, in
 * the instruction's own fixed order (elements at or past epi enter as zeros).  The waves' sums are then added in ascending wave order, starting from
 * wave 0's.  Only the two diagonal 16 x 16 tiles and the tile above the diagonal are formed (one tile for M <= 16); gram[i][a][b] and gram[i][b][a]
 * are both stored from the computed entry (min(a, b), max(a, b)), so they are the same bytes.
 *
 * Image function.  gram[i] depends on image i's values, M and epi only: not on n_images, on the image's position in the call or on the other
 * images.  A batch split over calls (offset pointers, the same hist_stride) gives the same bytes.  Nothing outside gram[0 .. n_images) is written.
 *
 * Limits: 1 <= n_rows <= NATINF_FIT_MAX_ROWS (M <= 32); rows (a HOST array, read before the call returns) strictly ascending and non-negative;
 * epi % 4 == 0 and 4 <= epi <= 2^24; 1 <= n_images <= 2^20; hist_stride >= n_images * epi and even (every history row is read in 16-byte
 * accesses); hist, noise, target and gram not NULL and 16-byte aligned.  Every violation is NATINF_EINVAL before anything is configured or launched
 * (so also on a machine with no GPU); NATINF_ELAUNCH when the runtime rejects the launch.
 */
#ifndef NATINF_FIT_H
#define NATINF_FIT_H

#include <stdint.h>
#include "natinf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NATINF_FIT_MAX_ROWS 30
/* Waves per image: the split points of the sum over the elements (above), a constant of the ABI, not of the launch. */
#define NATINF_FIT_WAVES 8

/* hist fp64 (device), rows int32 [n_rows] (host), noise / target fp32 [n_images][epi] (device) -> gram fp64 [n_images][M][M] (device). */
int natinf_fit_gram_f64(const double* hist, int64_t hist_stride, const int32_t* rows, int n_rows,
                        const float* noise, const float* target,
                        int64_t n_images, int64_t elems_per_image,
                        double* gram, natinf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NATINF_FIT_H */
