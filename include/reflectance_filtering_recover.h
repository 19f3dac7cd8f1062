/* reflectance_filtering_recover.h -- C ABI of librf_recover_hip.so (gfx950 / MI355X): the per-pixel
 * device operations of the reference trainer's relative estimation modes (--RS_est_mode rRelMean,
 * rRelMax, rRelY, rRelNorm): the recover layer (training/layers/recover_reflectance_shading_layer.py,
 * interpret_input_as_reflectance_intensity_relative), both boundary losses on its two tops
 * (boundary_loss_layer.py) with their gradient towards the network output, and the hinge loss's
 * gradient at judgement points folded into that gradient.
 *
 * The library is separate from librf_hip.so, librf_train_hip.so and librf_augment_hip.so and shares
 * no object with any of them.  It keeps NO state between calls - no tables, no side streams, no
 * allocation - so there is nothing to shut down.  Every entry takes DEVICE pointers only, stages
 * nothing, synchronises nothing, and enqueues all its work on `stream` (a hipStream_t, NULL = the
 * default stream), ordered like any kernel launch; the entries are safe to capture into a graph.
 * Return codes are numerically those of reflectance_filtering.h (RF_OK 0, RF_E_BADARG -1,
 * RF_E_UNSUPPORTED -2, RF_E_HIP -4); every refusal is decided on the host before any device work
 * and leaves its text in rf_recover_last_error() (thread-local).
 *
 * Buffers.  x [P][3] float32, interleaved B, G, R: the buffer rf_cnn_reflectance_f32 and
 * rf_train_cnn_points_backward_f32 take.  e [P] float32: the network's output at these pixels.
 * Pixel indices are 64-bit.  A pixel index outside [0, P) is the caller's error; it is NOT checked on
 * the device.  norm: 0 Mean, 1 Max, 2 Y, 3 Norm.
 *
 * Arithmetic, per pixel, every operation one correctly rounded float32 operation (the library is
 * built with -ffp-contract=off; divisions and the square root are true ones), EPS = FLT_EPSILON:
 *
 *   the floors are np.maximum(., EPS): a NaN in e stays NaN and reaches that pixel's outputs and grad_e
 *   (its boundary losses are 0, as the reference's masks leave them); no other pixel is touched by it
 *   Ri = max(e, EPS);  m = max(norm(R, G, B), EPS) with
 *       Mean ((R+G)+B)/3;  Max max(R,G,B);  Y (0.299f*R + 0.587f*G) + 0.114f*B;  Norm sqrt((R*R+G*G)+B*B)
 *   f = 1/m;  n_c = f*I_c;  reflectance refl_c = Ri*n_c
 *   Ri_inv = 1/Ri;  shading s = m*Ri_inv (the same in three channels)
 *   d refl_c / d e = n_c;  d s / d e = -Ri_inv*s  (the floors do not zero a derivative)
 *   lightness L = max(EPS, ((refl_R+refl_G)+refl_B)/3), d L / d refl_c = 1/3
 *   boundary loss of a blob (c0, c1, c2): v = ((c0+c1)+c2)/3;
 *       L1: loss -v where v < 0, v-1 where v > 1, else 0; slope -1, +1, 0
 *       L2: loss v*v where v < 0, (v-1)*(v-1) where v > 1, else 0; slope 2*v, 2*(v-1), 0
 *       per channel the blob's diff is d = ((slope / (float)count) / 3) * scale
 *   grad_e = ((((d_r*n_R + d_r*n_G) + d_r*n_B) + d_s*ds) + d_s*ds) + d_s*ds, ds = d s / d e: the
 *       reference's np.sum over the six channels reflectance R G B, shading 0 1 2.
 */
#ifndef REFLECTANCE_FILTERING_RECOVER_H
#define REFLECTANCE_FILTERING_RECOVER_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_RECOVER_VERSION 100
#define RF_RECOVER_NORM_MEAN 0
#define RF_RECOVER_NORM_MAX 1
#define RF_RECOVER_NORM_Y 2
#define RF_RECOVER_NORM_NORM 3
#define RF_RECOVER_PENALTY_L1 1
#define RF_RECOVER_PENALTY_L2 2

int rf_recover_version(void);
const char *rf_recover_last_error(void);

/* The recover layer at K listed pixels.  pixel [K] int64, or NULL = the pixels 0..K-1 (K <= P then).
 * Outputs, each optional (NULL = not wanted), row k belonging to pixel[k]: lightness [K],
 * reflectance [K][3] interleaved B, G, R like x, shading [K].
 *
 * K == 0 or P == 0 is RF_OK whatever the pointers, nothing written.  NULL x or e, negative P or K,
 * an unknown norm and pixel == NULL with K > P are RF_E_BADARG; P or K >= 2^31 is RF_E_UNSUPPORTED.
 */
int rf_recover_forward_f32(const float *x, const float *e, long long P, const long long *pixel,
                           long long K, int norm, float *lightness, float *reflectance,
                           float *shading, void *stream);

/* Both boundary losses over ALL P pixels (count = P) and their gradient towards e.
 *
 *   penalty            1 L1, 2 L2
 *   scale_reflectance, scale_shading   the loss weights: what Caffe puts into the two losses' diff
 *   loss_out [2] float64   the UNSCALED means of the reflectance and the shading boundary loss
 *   grad_e   [P] float32   every element written
 *
 * Loss sums are float64 over the float32 per-pixel losses in an order fixed by P and the plan alone:
 * workgroup g of G takes the passes g, g + G, ... of 256 consecutive pixels each; its thread t adds
 * the pixels 256 * pass + t of its passes in ascending order; the 256 partial sums are added pairwise
 * (t with t + 128, then t with t + 64, ... t with t + 1); the G rows (the workspace) are added in
 * ascending g by a second kernel and divided by (double)P.  No atomics: the same bits from run to
 * run, whatever the workspace held.
 *
 * workspace: rf_recover_boundary_workspace_bytes(P) bytes, 16-byte aligned; a NULL, smaller or
 * misaligned one is RF_E_BADARG.  P == 0 is RF_OK whatever the other pointers: no kernel runs,
 * grad_e is not touched, and loss_out, if given (non-NULL), is set to 0, 0 by a 16-byte memset node
 * on the stream.  NULL pointers, P < 0, an unknown norm or penalty and non-finite scales
 * are RF_E_BADARG; P >= 2^31 is RF_E_UNSUPPORTED.
 *
 * rf_recover_boundary_plan: out = {pixels per workgroup pass, workgroups, partial rows}; returns
 * RF_OK or the refusal of the entry for this P.  The workspace query returns 0 where the entry would
 * refuse P (and for P == 0).
 */
size_t rf_recover_boundary_workspace_bytes(long long P);
int rf_recover_boundary_plan(long long P, int out[3]);
int rf_recover_boundary_backward_f32(const float *x, const float *e, long long P, int norm,
                                     int penalty, float scale_reflectance, float scale_shading,
                                     double *loss_out, float *grad_e, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* The hinge loss's gradient at K judgement points, added into grad_e:
 *
 *   g = (scale * grad_l[k]) / 3;  grad_e[pixel[k]] += (g*n_R + g*n_G) + g*n_B
 *
 * grad_l [K] float32 is d loss / d lightness (what rf_train_whdr_hinge_points_f32 leaves in grad_r),
 * n_c the normalised image of the recover layer at pixel[k].  The call is a launch of its own,
 * ordered on the stream behind whatever wrote grad_e.  The listed pixels MUST be pairwise distinct:
 * that is the caller's duty (de-duplicated judgement points are), two equal indices race.
 *
 * K == 0 or P == 0 is RF_OK whatever the pointers.  NULL pointers, negative sizes, an unknown norm
 * and a non-finite scale are RF_E_BADARG; P or K >= 2^31 is RF_E_UNSUPPORTED.
 */
int rf_recover_hinge_scatter_f32(const float *x, const float *e, const float *grad_l,
                                 const long long *pixel, long long K, long long P, int norm,
                                 float scale, float *grad_e, void *stream);

#ifdef __cplusplus
}
#endif
#endif
