/* reflectance_filtering_train.h -- C ABI of librf_train_hip.so (gfx950 / MI355X): the two device
 * operations that fine-tuning the shipped 1x1 reflectance CNN on the WHDR hinge loss needs beyond
 * the forward pass of librf_hip.so (reflectance_filtering.h).
 *
 * The library is separate from librf_hip.so and shares no object with it.  It keeps NO state between
 * calls - no tables, no slots, no side streams, no allocation - so there is nothing to shut down, and
 * rf_shutdown() of the main library does not concern it.  Every entry takes DEVICE pointers only,
 * stages nothing, synchronises nothing, and enqueues all its work on `stream` (a hipStream_t, NULL =
 * the default stream), ordered like any kernel launch; the entries are safe to capture into a graph.
 * Return codes are numerically those of reflectance_filtering.h (RF_OK 0, RF_E_BADARG -1,
 * RF_E_UNSUPPORTED -2, RF_E_HIP -4); every refusal is decided on the host before any device work
 * and leaves its text in rf_train_last_error() (thread-local).
 *
 * tests/test_gpu_train_contract.py holds both device entries to these sentences with the runners of the
 * main library's four contract modules (cases: tests/train_cases.py): every buffer at odd residues
 * inside a guarded arena over a dirty workspace, behind a delay on a busy non-blocking side stream
 * (the call returns while the work in front of it is pending), captured once into a graph and replayed
 * on true inputs and on decoys - also after rf_shutdown() of the main library -, and over buffers
 * past byte 2^32 and at the largest admitted launch.
 */
#ifndef REFLECTANCE_FILTERING_TRAIN_H
#define REFLECTANCE_FILTERING_TRAIN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_TRAIN_VERSION 100
#define RF_TRAIN_CNN_NPARAMS 4513 /* = RF_CNN_NPARAMS: W0[32][3] b0[32] | 4 x (W[32][32] b[32]) | wf[160] bf */

int rf_train_version(void);
const char *rf_train_last_error(void);

/* WHDR hinge loss and its gradient at de-duplicated judgement points, one reflectance channel
 * (the arithmetic of the reference's training/layers/whdr_hinge_loss_layer.py, _whdr_hinge_single_img
 * and _eval_single_comparison, lightness of one channel as in whdr_layer.py).
 *
 *   r              [total] float32   reflectance at the packed points of ALL images
 *   point_offsets  [n+1]   int32     absolute offsets into r
 *   comps          [m][3]  int32     (index 1, index 2, darker); indices local to the image's points,
 *                                    darker 0 = about equal, 1 = point 1 darker, 2 = point 2 darker
 *   weights        [m]     float64   weight of each comparison
 *   comp_offsets   [n+1]   int32     absolute offsets into comps / weights
 *   inc_offsets    [total+1] int32   start of every point's incidence list in inc (absolute point index)
 *   inc            [2m]    int32     per point its comparisons in ascending comparison order, each entry
 *                                    2 * (k - comp_offsets[image]) + side (side 0: the point is index 1);
 *                                    a comparison whose two ends are one point appears twice
 *   loss_out       [n]     float64   per image sum(w * l) / sum(w); 0 for an image without comparisons
 *                                    or with a zero weight sum
 *   grad_r         float32, written for exactly the points [point_offsets[0], point_offsets[n]), at
 *                  their absolute positions: the gradient of the MEAN of loss_out over the n images
 *                  (every term divided by its image's weight sum and by n; 0 in weightless images)
 *
 * The offsets are absolute and the base pointers are passed unchanged, so the consecutive images
 * [i0, i0 + n) of a packed set are selected by passing point_offsets + i0, comp_offsets + i0 and n.
 *
 * Per comparison, in float32: L = max(FLT_EPSILON, r) (the clamp does not zero the derivative),
 * L2inv = 1 / L2, y = L1 * L2inv, dy/dL1 = L2inv, dy/dL2 = -y * L2inv.  The hinge borders are formed
 * in double from delta and margin and rounded to float32.  darker 1: loss max(0, y - 1/(1+delta+margin));
 * darker 2: max(0, (1+delta+margin) - y); darker 0 with margin <= delta: max(0, y - b, 1/b - y) with
 * b = 1 + delta - margin; darker 0 with margin > delta: max(1/b - y, y - b), its slope +1 where y > 1,
 * else -1.  Any other darker value is the caller's error (such a comparison adds nothing here).
 * The float32 loss l and slope dl/dy * dy/dL of a comparison are multiplied by its float64 weight
 * in double (with -ffp-contract=off: a product, then a sum).
 * ALL comparisons passed are evaluated: the reference's random subsample above 1,500 comparisons
 * per image is not mirrored, and its `ratio` / `eval_dense` selection is the caller's, done when the
 * arrays are built.
 *
 * Every sum is float64 in an order fixed by the arrays and never by the launch: per image, partial
 * sum t (t = 0..255) takes the comparisons t, t + 256, t + 512, ... of the image in ascending order,
 * and the 256 partial sums are added pairwise (t with t + 128, then t with t + 64, ... t with t + 1);
 * per point, the terms of its incidence list in list order.  No atomics.  Results are the same bits
 * from run to run.
 *
 * n == 0 is RF_OK whatever the pointers; NULL pointers, n < 0, negative or non-finite delta / margin
 * are RF_E_BADARG; n >= 2^24 is RF_E_UNSUPPORTED (one workgroup of 256 per image in one launch).
 */
int rf_train_whdr_hinge_points_f32(const float *r, const int *point_offsets, const int *comps,
                                   const double *weights, const int *comp_offsets,
                                   const int *inc_offsets, const int *inc, int n, double delta,
                                   double margin, double *loss_out, float *grad_r, void *stream);

/* Backward pass of the CNN at P points: grad_w[j] = d/dw_j sum_p grad_r[p] * r(x_p; w).
 *
 *   x        [P][3] float32  network inputs, interleaved B, G, R: the RF_CNN_NHWC_BGR buffer that
 *                            rf_cnn_reflectance_f32 takes as [1][1][P][3]
 *   weights  [4513] float32  the layout of rf_cnn_reflectance_f32
 *   grad_r   [P]    float32  d loss / d r at the points
 *   grad_w   [4513] float32  out, same layout as weights
 *
 * The forward pass is recomputed per point with the float32 FMA chains of the forward kernels (five
 * ReLU layers, the 160-wide concatenation of the post-ReLU activations, the fuse layer, the sigmoid)
 * and back-propagated with sigma' = r (1 - r); the ReLU derivative is 0 where the pre-activation
 * is <= 0.  Sums over points: workgroup g of G (rf_train_cnn_points_plan) takes the passes g, g + G,
 * ... of 64 consecutive points each and sums them in that order (the 32 x 32 weight matrices in
 * float32 through the exact-f32 matrix instruction, two points per step ascending; biases, W0 and
 * the fuse weights in float64, point by point ascending); the G partial gradients (float64 rows
 * of the workspace) are then added in float64 in ascending g and rounded to float32 once.  No atomics:
 * the result is the same bits from run to run and does not depend on what the workspace held.
 *
 * workspace: rf_train_cnn_points_workspace_bytes(P) bytes, 16-byte aligned; a smaller or misaligned
 * one is RF_E_BADARG.  P == 0 is RF_OK whatever the pointers (grad_w is then NOT written); NULL
 * pointers and P < 0 are RF_E_BADARG; P >= 2^31 is RF_E_UNSUPPORTED (32-bit point indices in one launch).
 *
 * rf_train_cnn_points_plan: out = {points per workgroup pass, workgroups, partial-gradient rows};
 * returns RF_OK or the refusal of the entry for this P.  The workspace query returns 0 where the
 * entry would refuse P (and for P == 0).
 */
size_t rf_train_cnn_points_workspace_bytes(long long P);
int rf_train_cnn_points_plan(long long P, int out[3]);
int rf_train_cnn_points_backward_f32(const float *x, const float *weights, const float *grad_r,
                                     long long P, float *grad_w, void *workspace,
                                     size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
