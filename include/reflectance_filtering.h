/*
 * reflectance_filtering.h -- C ABI of librf_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the three native calls on the reference's hot path.
 * Every entry point takes plain device pointers and sizes, runs asynchronously
 * on the HIP stream it is given (hipStream_t passed as void*; NULL = the null
 * stream), never allocates or synchronises on the launch path once its
 * parameter tables are cached, and never throws: it returns RF_OK or a negative
 * RF_E* code, and rf_last_error() returns the calling thread's message.
 *
 * There is no CPU fallback in this library.  Images are uint8, interleaved
 * (H x W x C), tightly packed, batched along the leading dimension n; every
 * image of a batch is filtered independently (no inter-image or inter-GPU
 * traffic; shard batches across GPUs by giving each process its own slice).
 *
 * Buffers (held for every entry by tests/test_gpu_buffer_contract.py, with every buffer at odd and
 * even offsets from a 256-byte boundary, guard bytes around each and 0x00 / 0xA5 / 0xFF in a workspace
 * of exactly the queried size):
 *   - an image, point, weight or result buffer may start at any address that is a multiple of its
 *     element size (uint8 images at any byte: a slice of a batch of odd-sized images is a valid
 *     argument); only a workspace has an alignment rule - 16 bytes, stated with each entry - and where
 *     an entry says "scratch" it means this;
 *   - the contents of a workspace on entry are arbitrary: a call initialises every counter, flag and
 *     table it reads, so a workspace need not be cleared and may be reused call after call;
 *   - a call writes nothing outside its outputs and the workspace_bytes bytes it was given (the size
 *     query's answer is always enough), and no result depends on the bytes around an input;
 *   - a call leaves its inputs alone, except where an entry says otherwise (dst == src of the guided
 *     filter, `raw` of rf_png_unfilter_ragged_u8).
 *
 * Streams (held for every entry by tests/test_gpu_stream_contract.py, on a non-blocking side stream kept
 * busy in front of the call, with inputs that arrive on that stream just before it and are overwritten
 * on it right after it):
 *   - everything a call enqueues - helper launches, staging copies, work on a side stream of the
 *     library - is ordered after what `stream` holds at the call and before what is enqueued on it
 *     afterwards; a parameter table that is uploaded on a stream of the library is resident before the
 *     call launches anything that reads it;
 *   - a call whose parameter tables are cached returns without waiting for the device, however much
 *     work is queued in front of it, unless its entry says "SYNCHRONISES THE STREAM"; such an entry waits
 *     once, for its own stream alone - never for the work of another non-blocking stream (rf_jbf_f32
 *     uploads its tables with two blocking copies on the null stream after its wait: like every use of
 *     the null stream they are ordered against streams created WITHOUT hipStreamNonBlocking);
 *   - what the library keeps per caller stream (side streams of the guided filter, vote bytes of
 *     rf_jbf_u8, packed-weight slots of the CNN: 16 each) may be used from more streams than are kept:
 *     a further stream is served by a recycled idle entry or by a route that needs none.
 *
 * Graphs (held for every entry by tests/test_gpu_capture_contract.py: one call captured on a side stream in
 * the default capture mode, after a warm eager call on that stream, and replayed over changed inputs and a
 * dirty workspace):
 *   - on a stream that is being captured into a graph every entry does one of two things.  Capturable:
 *     rf_jbf_u8, rf_gf_u8, rf_gf_ex_u8, rf_gf_f32, rf_colorize_srgb_u8, rf_whdr_f32, rf_whdr_points_u8,
 *     rf_cnn_pack_weights and the two rf_cnn_reflectance_packed entries - the call returns RF_OK and none
 *     of its work runs before a replay.  Refusing: every entry that
 *     says "SYNCHRONISES THE STREAM", on every route it has, and the raw-weight rf_cnn_reflectance_u8 and
 *     rf_cnn_reflectance_f32 - the call returns RF_E_UNSUPPORTED before anything is enqueued or written, the
 *     message names the entry and the capture, and the capture stays valid and the stream usable;
 *   - a replay reads its buffers - inputs and workspace - as they are at replay time, not as they were at
 *     the capture; it initialises whatever it reads of the workspace, like an eager call, and writes nothing
 *     but the call's outputs and its workspace.  The graph holds the addresses of the call's buffers: they
 *     stay allocated while it can be replayed;
 *   - a graph also holds addresses of what the library keeps (parameter tables, the vote bytes of its
 *     capture stream): destroy every graph that captured a library call before rf_shutdown, and those that
 *     captured rf_jbf_u8 before rf_jbf_release_scratch; replays of graphs that captured rf_jbf_u8 on one
 *     stream are serialised.  After either call everything is rebuilt on demand, by every
 *     entry.
 *
 * Sizes (held by tests/test_gpu_size_contract.py, whose buffers pass 2^31 and 2^32 bytes, and by
 * tests/test_launch_limits_abi.py.  Within 32 GiB per call, one-channel 8-bit buffers pass pixel index 2^32
 * too - those of the colourise entries 2^31, those of rf_gf_ragged_u8 2^30 - and float buffers element
 * index 2^31, those of the CNN entries 2^32):
 *   - n, h, w and the counts are ints; every offset into a caller's buffer is formed in 64 bits, so a
 *     buffer may be as large as the device holds, up to these caps: 2^60 pixels in a list of
 *     rf_jbf_ragged_u8 or rf_jbf_points_ragged_u8, 2^58 in one of rf_gf_ragged_u8, 2^46 in one of the
 *     ragged colourise entries (and 3 h w < 2^32 per image); w < 2^27 for the guided filter; raw stream and
 *     pixels below 2^31 per image of rf_png_unfilter_ragged_u8, a stream bound below 2^31 for
 *     rf_png_deflate_ragged_u8;
 *   - a call whose work does not fit one launch is refused with RF_E_UNSUPPORTED ("... for one launch";
 *     the ragged colourise entries and the unpack grid of rf_png_unfilter_ragged_u8 say "... than one
 *     grid takes")
 *     before any device work (rf_jbf_u8 alone may have uploaded the parameter tables of its sigmas by
 *     then; it launches nothing): the runtime takes no launch of 2^32 work-items or more.  That is 4,194,303
 *     tiles of 64 x 64 for rf_jbf_u8 and rf_jbf_ragged_u8 (17 gigapixels of whole tiles; for a ragged
 *     list every image counts ceil(h / 64) ceil(w / 64) tiles, so 4,194,303 images at most);
 *     16,777,215 stage-1 strips, 64-row blocks or column blocks for rf_gf_ragged_u8; 16,777,215
 *     workgroups and 8,388,607 images for the ragged colourise entries; 67,108,860 waves for the point
 *     entries (a wave takes 64 / n_params points of one group of sigma_space, at most); 67,108,863 for n
 *     of rf_whdr_f32 and n * n_sets of rf_whdr_points_u8; 4,194,303 images and 16,777,215 blocks of 4096
 *     pixels for rf_png_unfilter_ragged_u8; n <= 65535 for rf_colorize_srgb_u8, rf_jbf_f32 and the
 *     untiled route of rf_jbf_u8 (RF_JBF_FORCE_GENERIC, radius above 468).  The CNN entries run a
 *     grid of fixed size.  rf_gf_u8, rf_gf_ex_u8 and rf_gf_f32 split a batch themselves: they work in
 *     chunks of at most 16383 (8-bit kernels) or 65535 images (float kernels), and of no more images
 *     than their launches take, however large the workspace is; they refuse only an image that is
 *     itself too large for a launch (16,777,215 / src_cn blocks of 64 rows, for instance).
 */
#ifndef REFLECTANCE_FILTERING_H
#define REFLECTANCE_FILTERING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_VERSION 103 /* 0.1.3 */

/* return codes */
#define RF_OK 0
#define RF_E_BADARG (-1)      /* NULL pointer, non-positive size, sigma handling is OpenCV's (<=0 -> 1) */
#define RF_E_UNSUPPORTED (-2) /* channel count / radius / border outside what is implemented */
#define RF_E_WORKSPACE (-3)   /* workspace too small for one image */
#define RF_E_HIP (-4)         /* a HIP runtime call failed; see rf_last_error() */

/* border types, numerically equal to cv::BorderTypes */
#define RF_BORDER_CONSTANT 0
#define RF_BORDER_REPLICATE 1
#define RF_BORDER_REFLECT 2
#define RF_BORDER_WRAP 3
#define RF_BORDER_REFLECT_101 4
#define RF_BORDER_DEFAULT RF_BORDER_REFLECT_101

/* rf_jbf_u8 flags */
#define RF_JBF_TRUE_DIVISION 1 /* dst = sum / wsum; default is OpenCV's sum * (1.f / wsum) */
#define RF_JBF_FORCE_GENERIC 2 /* use the untiled global-memory kernel (debug / cross-check) */
#define RF_JBF_GREY_AS_BGR 4    /* a 1-channel joint counts as 3 equal channels, i.e. what cv2.imread makes of a
                                 grey PNG (colour distance 3*|d|); with a 1-channel src the 1-channel result
                                 equals every channel of the 3-channel one */
/* any other flag bit is rejected (RF_E_BADARG); test and benchmark switches live in
   reflectance_filtering_debug.h */

int rf_version(void);
const char *rf_last_error(void);
/* Frees what the library holds: the per-device parameter tables (colour LUTs, tap tables), the
   packed-weight slots of rf_cnn_reflectance_u8 and rf_cnn_reflectance_f32, the guided filter's side
   streams and the scratch of rf_jbf_release_scratch.  Call it with no library work in flight and no
   captured graph of a library call left to replay ("Graphs" above); every entry rebuilds what it
   needs at its next call. */
int rf_shutdown(void);
/* Frees the scratch rf_jbf_u8 keeps from call to call (one vote byte per 64x64 tile of its largest
   launch, per device and stream, for at most 16 streams).  Call it with no rf_jbf_u8 work in flight
   and no captured graph of such a call left to replay; rf_shutdown does the same.  Graphs that
   captured rf_jbf_u8 on one stream share that stream's bytes: serialise their replays
   (INTEGRATION.md). */
int rf_jbf_release_scratch(void);

/*
 * Joint bilateral filter, 8-bit.
 * Replaces  cv2.ximgproc.jointBilateralFilter(joint, src, d, sigmaColor, sigmaSpace[, borderType])
 * as called at /root/reference/filter_reflectance.py:60-64 (d = -1).
 *   joint  n*h*w*joint_cn   device, joint_cn in {1,3}
 *   src    n*h*w*src_cn     device, src_cn   in {1,3}
 *   dst    n*h*w*src_cn     device, must not overlap joint or src
 *   d <= 0 -> radius = cvRound(1.5*sigma_space), else radius = d/2; radius >= 1
 * Per pixel the taps are accumulated in OpenCV's order (row-major over the
 * disk, float32, separately rounded multiply and add), so the uint8 result is
 * bit-identical to the restated CPU algorithm.
 */
int rf_jbf_u8(const uint8_t *joint, const uint8_t *src, uint8_t *dst, int n, int h, int w,
              int joint_cn, int src_cn, int d, double sigma_color, double sigma_space, int border,
              int flags, void *stream);

/*
 * rf_jbf_u8 over images of different sizes (IIW photos come in many shapes) in one call.
 *   joint, src, dst  the n images tightly packed one after another: image i starts at pixel
 *                  sum over j < i of heights[j] * widths[j] (offsets are formed in 64 bits) and is
 *                  heights[i] rows of widths[i] pixels; dst must not overlap joint or src (judged
 *                  on the summed pixel count)
 *   heights, widths  n ints each, HOST memory: every entry must be > 0 (RF_E_BADARG otherwise, and
 *                  for a NULL array)
 *   workspace      device scratch, 16-byte aligned, of at least rf_jbf_ragged_workspace_bytes(n,
 *                  heights, widths, joint_cn, src_cn, d, sigma_space, flags) bytes: 32 bytes per 64x64
 *                  tile of every image (ceil(h/64) * ceil(w/64) each), rounded up to 256; 0 = arguments
 *                  the call refuses.  A NULL, misaligned or smaller workspace is RF_E_BADARG.
 * The bytes written for image i are, byte for byte, what rf_jbf_u8(n = 1, heights[i], widths[i], ...)
 * writes with the same other arguments; sigma, radius, flag, channel and border rules and refusals
 * are rf_jbf_u8's; n == 0 is RF_OK whatever the pointers are.
 * Radius <= 52 (the paper's c20 s22 and c15 s28 among them): the tiles of all images run in one
 * launch per tile shape - at most four - from one record per tile (first pixel, height, width, tile
 * origin), staged in the workspace by one copy.  Radius 53..468: the tiles of all images run in ONE
 * launch of tap-row slabs, from the same records staged the same way.  For that copy the call
 * SYNCHRONISES THE STREAM once, on both routes (its own stream only: it waits for no other stream's
 * work).
 * Every other route of rf_jbf_u8 (radius 469 and up, RF_JBF_FORCE_GENERIC, a device whose LDS probe
 * fails, the "jbf_tune" debug switch) is taken by calling rf_jbf_u8 once per image: the same bytes
 * with n launches and no synchronisation.  Either way the call is refused (RF_E_UNSUPPORTED) on a
 * stream that is being captured into a graph.
 */
size_t rf_jbf_ragged_workspace_bytes(int n, const int *heights, const int *widths, int joint_cn,
                                     int src_cn, int d, double sigma_space, int flags);
int rf_jbf_ragged_u8(const uint8_t *joint, const uint8_t *src, uint8_t *dst, int n,
                     const int *heights, const int *widths, int joint_cn, int src_cn, int d,
                     double sigma_color, double sigma_space, int border, int flags, void *workspace,
                     size_t workspace_bytes, void *stream);

/*
 * Guided filter, 8-bit, colour guide.
 * Replaces  cv2.ximgproc.guidedFilter(guide, src, radius, eps)  as called at
 * /root/reference/filter_reflectance.py:67-70 (radius = int(sigma_spatial), eps = sigma_color).
 *   guide  n*h*w*3        device (guide_cn must be 3: cv2.imread always yields 3 channels)
 *   src    n*h*w*src_cn   device, src_cn in {1,3}
 *   dst    n*h*w*src_cn   device; may alias src
 *   radius 0..4096 (int(sigma_spatial) is a free parameter of the reference's tool): radii up to
 *   128 run the 8-bit kernels (exact uint32 window sums); larger ones run the float kernels of
 *   rf_gf_f32 on float copies of the images kept in the workspace, each pass rounded to uint8 like
 *   convertTo(CV_8U) - the same bytes (on 8-bit data the float path's double window sums are the
 *   same exact integers).  rf_gf_workspace_bytes sizes the workspace for the radius it is given.
 *   iterations >= 1: the filter is applied `iterations` times with the same guide, the uint8
 *   result of one pass being the src of the next (the reference's "3x GF" chain of CLI runs).
 *   workspace: device scratch of at least rf_gf_workspace_bytes(1, ...) bytes, 16-byte aligned (not
 *   checked: its parts are laid out at multiples of 16 bytes from its start, and the float route
 *   keeps double row sums among them);
 *   larger workspaces let more images of the batch be in flight at once.
 *   stream: all work is ordered after what `stream` holds at the call and before what is
 *   enqueued on it afterwards; inside, half of a batch may run on a side stream of the library
 *   that is forked from and joined back into `stream` with events (graph capture keeps working).
 *   Side streams are per caller stream (at most 16 are kept), so concurrent callers on different
 *   streams - eager or capturing - never meet on one.
 */
size_t rf_gf_workspace_bytes(int n, int h, int w, int guide_cn, int src_cn, int radius);
int rf_gf_u8(const uint8_t *guide, const uint8_t *src, uint8_t *dst, int n, int h, int w,
             int guide_cn, int src_cn, int radius, double eps, int iterations, void *workspace,
             size_t workspace_bytes, void *stream);

/*
 * Guided filter, 8-bit, with flags.  flags == 0 is rf_gf_u8 (the same results and the same
 * refusals).
 *   RF_GF_GREY_AS_BGR  guide is n*h*w*1 (guide_cn must be 1, src_cn 1 or 3): each guide byte stands
 *     for three equal channels, i.e. what cv2.imread makes of a grey PNG such as the CNN's `-r.png`
 *     - the reference tool's GF(CNN, CNN) recipe (its filter_reflectance.py:135-137).  The result is
 *     byte for byte rf_gf_u8 on the guide replicated to 3 channels; the grey guide is read at one
 *     byte per pixel and stage 1 box-sums 2 + 2 x src_cn quantities instead of 9 + 4 x src_cn.
 *     This is NOT cv2.ximgproc.guidedFilter on a 1-channel guide: for one guide channel OpenCV
 *     inverts var + eps as a scalar, whereas three equal channels with eps*I on the diagonal go
 *     through the 3x3 inverse (and its small-eps determinant rule) - different floats.  Only the
 *     second is implemented.
 *   Refused: guide_cn == 3 with the flag and any unknown flag bit (RF_E_BADARG); guide_cn == 1
 *   without the flag (RF_E_UNSUPPORTED, as rf_gf_u8).  The workspace is sized by
 *   rf_gf_workspace_bytes as for a colour guide (a grey guide needs no more).
 */
#define RF_GF_GREY_AS_BGR 1
int rf_gf_ex_u8(const uint8_t *guide, const uint8_t *src, uint8_t *dst, int n, int h, int w,
                int guide_cn, int src_cn, int radius, double eps, int iterations, int flags,
                void *workspace, size_t workspace_bytes, void *stream);

/*
 * rf_gf_ex_u8 over images of different sizes in one call (a list of reflectance maps through
 * GF(CNN, CNN) or GF(CNN, flat)).
 *   guide, src, dst  the n images tightly packed one after another: image i starts at pixel
 *                  sum over j < i of heights[j] * widths[j] (offsets are formed in 64 bits) and is
 *                  heights[i] rows of widths[i] pixels.  Overlap is judged on the summed pixel count:
 *                  dst may equal src, may not partially overlap it and may not overlap guide; guide
 *                  may equal src (a map that guides itself).
 *   heights, widths  n ints each, HOST memory: every entry must be > 0 (RF_E_BADARG otherwise, and
 *                  for a NULL array)
 *   workspace      device scratch, 16-byte aligned, of at least rf_gf_ragged_workspace_bytes(n,
 *                  heights, widths, guide_cn, src_cn, radius, flags) bytes; 0 = arguments the call
 *                  refuses.  A NULL, misaligned or smaller workspace is RF_E_BADARG.
 * The bytes written for image i are, byte for byte, what rf_gf_ex_u8(n = 1, heights[i], widths[i], ...)
 * writes with the same other arguments; channel, flag, radius and overlap rules and refusals are
 * rf_gf_ex_u8's (the debug options it refuses with a grey guide included); n == 0 is RF_OK whatever
 * the pointers are.
 * Ragged route - src_cn == 1, radius 1..128, every image below 2^28 pixels: stage 1, the row walk and
 * the column walk run ONCE per pass over all images (three launches per pass, on `stream` alone), each
 * workgroup finding its image through a table in the workspace: 48 bytes per image, 16 bytes per work
 * item (stage 1: strip x segment; row walk: 64-row block; column walk: 16-column block, in 8 equal
 * runs), rounded up to 256, followed by the row states (32 * ceil(w / 16) * h bytes per image) and
 * alpha/beta (16 bytes per pixel) of the WHOLE list: a long list is split by the caller.  The table is
 * staged by one copy, for which the call SYNCHRONISES THE STREAM once.
 * Fallback route - src_cn == 3, radius 0, radius above 128 (and the debug options that select another
 * stage-2 form): rf_gf_ex_u8 once per image on a workspace sized for the most demanding image: the
 * same bytes with n calls and no synchronisation.
 * Either way the call is refused (RF_E_UNSUPPORTED) on a stream that is being captured into a graph,
 * before anything is enqueued.
 */
size_t rf_gf_ragged_workspace_bytes(int n, const int *heights, const int *widths, int guide_cn,
                                    int src_cn, int radius, int flags);
int rf_gf_ragged_u8(const uint8_t *guide, const uint8_t *src, uint8_t *dst, int n,
                    const int *heights, const int *widths, int guide_cn, int src_cn, int radius,
                    double eps, int iterations, int flags, void *workspace, size_t workspace_bytes,
                    void *stream);

/*
 * 1x1 CNN reflectance predictor on uint8 BGR images.
 * Replaces  caffe.Net(network_definition.prototxt, TEST, weights=learned_weights.caffemodel),
 * blobs['images'] <- imgCV2_to_caffeBlob(image), forward(), blobs['reflectance_intensity']
 * (/root/reference/decompose_with_trained_CNN.py:57-69, 82-95, 100-106).
 *   bgr        n*h*w*3 uint8 device (cv2.imread layout)
 *   r_out      n*h*w float32 device or NULL: sigmoid output in (0,1)
 *   r_u8_out   n*h*w uint8 device or NULL: trunc(r*255), the bytes of `<base>-r.png`
 *              (/root/reference/image_utils.py:63-68)
 *   weights    4513 float32 on the device:
 *              W0[32][3] b0[32] | 4 x (W[32][32] b[32]) | wf[160] bf[1]
 *   srgb_lut   256 float32 on the device: linear value of each sRGB byte
 * The call packs the weights into a slot the library keeps per (device, stream), so it is refused
 * (RF_E_UNSUPPORTED) on a stream that is being captured into a graph, before anything is enqueued:
 * graphs use the pair below.
 */
#define RF_CNN_NPARAMS 4513
#define RF_CNN_NPACKED 4673 /* floats of rf_cnn_pack_weights' output */
int rf_cnn_reflectance_u8(const uint8_t *bgr, float *r_out, uint8_t *r_u8_out, int n, int h, int w,
                          const float *weights, const float *srgb_lut, void *stream);
/*
 * The same forward pass split the way pycaffe splits it: rf_cnn_pack_weights is the net-load step
 * (caffe.Net(prototxt, TEST, weights=...), /root/reference/decompose_with_trained_CNN.py:104-106),
 * done once per set of weights; rf_cnn_reflectance_packed_u8 is forward() on a loaded net
 * (:86-92).  The library keeps no state for this pair, so it can be captured into a HIP graph and
 * used from any number of streams.  rf_cnn_reflectance_u8 above is pack + forward in one call,
 * with the packed copy in a small library-owned table keyed by (device, stream) whose slots are
 * recycled; it is refused (RF_E_UNSUPPORTED) on a stream that is being captured - a graph would
 * keep a slot's address after the slot has moved on - so graphs use the pair.
 *   weights  4513 float32 on the device, layout as above
 *   packed   RF_CNN_NPACKED float32 on the device, caller-owned: the weights in the order the
 *            kernel streams them, the 160 fuse weights twice each (opaque; valid for this library
 *            version)
 */
int rf_cnn_pack_weights(const float *weights, float *packed, void *stream);
int rf_cnn_reflectance_packed_u8(const uint8_t *bgr, float *r_out, uint8_t *r_u8_out, int n, int h,
                                 int w, const float *packed, const float *srgb_lut, void *stream);

/*
 * The same network on float32 LINEAR images: whatever floats a Caffe blob holds (MIT Intrinsic, MPI
 * Sintel, HDR / EXR / RAW data, the npz and movie inputs of the reference's trainer), not only the
 * 256 values that 8-bit sRGB pixels decode to.  Only the input stage differs from the u8 entries:
 * the network's input is the float as it is, where they look a byte up in srgb_lut.
 *   x        n*h*w*3 float32 device, linear, nominally 0..1 (nothing is clamped), in one of two layouts:
 *            RF_CNN_NCHW_RGB  planar [n][3][h][w], channels R, G, B: net.blobs['images'].data
 *            RF_CNN_NHWC_BGR  interleaved [n][h][w][3], channels B, G, R: the float twin of `bgr`
 *   r_out, r_u8_out, weights, packed   as for the u8 entries
 * Contract: for an x whose values are all table levels, x = srgb_lut[byte], both entries write the
 * SAME BITS (r_out and r_u8_out) as rf_cnn_reflectance_u8 / _packed_u8 on the corresponding bytes;
 * a pixel's result depends on its three values only, not on its place, the layout or the entry.
 * Non-finite inputs (NaN, +-inf): no input value is used as an index, so they cannot make the call
 * read or write outside its buffers; the outputs of the pixels that hold them are unspecified, every
 * other pixel of the call is unaffected, and the call returns RF_OK.
 * Rules: those of the u8 twins - n == 0 is RF_OK whatever the pointers are; either output may be NULL,
 * not both; n < 0, h <= 0, w <= 0 and NULL inputs are RF_E_BADARG; nothing is synchronised;
 * rf_cnn_reflectance_f32 re-packs the weights on the caller's stream into the library's per-stream
 * slot and is refused on a capturing stream, rf_cnn_reflectance_packed_f32 keeps no state and can be
 * captured.  Refused in addition, before any device work (RF_E_BADARG): an unknown layout; r_out or
 * r_u8_out overlapping x (a pixel is read long after others were written); n*h*w of 2^48 or more.
 * Images of different sizes go through packed one after another as ONE image, n = 1, h = 1,
 * w = total pixels: interleaved [1][1][P][3], planar three planes of P values [1][3][1][P].
 */
#define RF_CNN_NCHW_RGB 0
#define RF_CNN_NHWC_BGR 1
int rf_cnn_reflectance_f32(const float *x, float *r_out, uint8_t *r_u8_out, int n, int h, int w,
                           int layout, const float *weights, void *stream);
int rf_cnn_reflectance_packed_f32(const float *x, float *r_out, uint8_t *r_u8_out, int n, int h,
                                  int w, int layout, const float *packed, void *stream);

/*
 * Colourised reflectance and shading PNG bytes of decompose_image.
 * Replaces the host numpy chain  iu.colorize(reflectance_gray, image)  +  iu.imwrite(..., sRGB=True)
 * of both results (/root/reference/decompose_with_trained_CNN.py:121-128,
 * /root/reference/image_utils.py:42-49, 60-92) for a batch that is already on the device:
 *   shading = mean_c(bgr) / r ; reflectance = bgr / max(shading, 1e-3)          (float64)
 *   each: if max > 1: clip(x / percentile(x, 99.9, 'lower'), 0, 1); rgb_to_srgb; trunc(x * 255)
 *   r must be >= +0.  r == 0 makes the shading +inf (a black pixel: 0/0 = NaN, and NaN
 *   reflectance).  As in numpy, max is NaN for a result that holds a NaN, `max > 1` fails and that
 *   result is written WITHOUT normalisation: NaN -> byte 0, values above 1 keep counting
 *   srgb_steps up to byte 255.  Where numpy's trunc(x * 255) would be >= 256 (x above ~1.087)
 *   its uint8 cast overflows and the reference's byte depends on the platform: unspecified
 *   (this library writes 255).
 *   bgr          n*h*w*3 uint8 device        r   n*h*w float32 device (the CNN output)
 *   refl_out     n*h*w*3 uint8 device or NULL (bytes of `<base>-r_colorized.png`, BGR order)
 *   shading_out  n*h*w   uint8 device or NULL (bytes of `<base>-s_colorized.png`)
 *   k_refl, k_shading  0-based rank of the 99.9-percentile ('lower') among the 3*h*w resp. h*w
 *                values of one image, computed by the caller with numpy's own index rule
 *   srgb_steps   255 float64 on the device: srgb_steps[k-1] = smallest x > 0.0031308 with
 *                trunc(((1.055*x)^(1/2.4) - 0.055) * 255) >= k under the HOST's pow (all finite;
 *                k >= 247 lie above 1);
 *                this makes the bytes exact for the libm the reference would have used
 *   workspace    device scratch, rf_colorize_workspace_bytes(n) bytes, 16-byte aligned (not checked:
 *                it holds the selection state of each image - 64-bit keys and ranks, a 256-bin
 *                histogram - which the call initialises itself)
 */
size_t rf_colorize_workspace_bytes(int n);
int rf_colorize_srgb_u8(const uint8_t *bgr, const float *r, uint8_t *refl_out, uint8_t *shading_out,
                        int n, int h, int w, unsigned long long k_refl, unsigned long long k_shading,
                        const double *srgb_steps, void *workspace, size_t workspace_bytes,
                        void *stream);

/*
 * rf_colorize_srgb_u8 over images of different sizes in one call: the percentile, the `max > 1`
 * test and the NaN rule stay per image.
 *   bgr, r, refl_out, shading_out  the n images tightly packed one after another: image i starts at
 *                pixel sum over j < i of heights[j] * widths[j] (offsets are formed in 64 bits);
 *                either output may be NULL, not both
 *   heights, widths, k_refl, k_shading  n entries each, HOST memory: every size > 0, every image
 *                with 3 * h * w < 2^32 (RF_E_UNSUPPORTED otherwise: the histogram counters are 32 bits
 *                wide), k_refl[i] < 3 * h_i * w_i and k_shading[i] < h_i * w_i the ranks of image i
 *   workspace    device scratch, 16-byte aligned, of at least rf_colorize_ragged_workspace_bytes(n,
 *                heights, widths) bytes: 40 bytes per image rounded up to 256 (the image table) plus
 *                what rf_colorize_workspace_bytes(n) asks for; 0 = arguments the call refuses.  It may
 *                be reused call after call: a call clears everything it reads.
 * The bytes written for image i are, byte for byte, those of rf_colorize_srgb_u8(n = 1, heights[i],
 * widths[i], k_refl[i], k_shading[i], ...) on that image alone; n == 0 is RF_OK whatever the
 * pointers are.  A workgroup takes one chunk of consecutive pixels of one image - one chunk length
 * per call, chosen from the summed pixel count - so the 18 launches of the uniform entry serve the
 * whole list.  The image table is staged in the workspace by one copy on `stream`, and for that copy
 * the call SYNCHRONISES THE STREAM once; it is refused (RF_E_UNSUPPORTED) on a stream that is being
 * captured into a graph.  rf_colorize_srgb_u8 above synchronises nothing and stays capturable.
 * Every refusal (NULL pointers, n < 0, bad sizes or ranks - the message names the image -, more
 * workgroups than one grid takes, RF_E_WORKSPACE for a workspace that is too small) is decided
 * before any device work.
 */
size_t rf_colorize_ragged_workspace_bytes(int n, const int *heights, const int *widths);
int rf_colorize_ragged_srgb_u8(const uint8_t *bgr, const float *r, uint8_t *refl_out,
                               uint8_t *shading_out, int n, const int *heights, const int *widths,
                               const unsigned long long *k_refl, const unsigned long long *k_shading,
                               const double *srgb_steps, void *workspace, size_t workspace_bytes,
                               void *stream);

/*
 * rf_colorize_ragged_srgb_u8 of an 8-bit reflectance map - a filtered `-r.png` that is on the device
 * already: the reflectance of a pixel is the float32 nearest to byte / 255 (__fdiv_rn((float)byte,
 * 255.0f), the convention of rf_whdr_points_u8), formed in registers by the eight histogram passes
 * and the write pass, which read one byte per pixel; no float copy of the map exists.
 *   r8           one uint8 per pixel, packed like bgr.  Byte 0 is r == 0 of rf_colorize_srgb_u8:
 *                the shading is +inf, a black pixel gives NaN, and a result holding a NaN is written
 *                without normalisation.
 * Every other argument, the workspace (rf_colorize_ragged_workspace_bytes), the refusals - all
 * decided before any device work -, the refusal on a capturing stream and n == 0 are those of
 * rf_colorize_ragged_srgb_u8, and like it the call SYNCHRONISES THE STREAM once (for the copy of the
 * image table).  The bytes written are, for every input,
 * those of rf_colorize_ragged_srgb_u8 given the float32 array (float)r8[i] / 255.0f.
 */
int rf_colorize_ragged_r8_srgb_u8(const uint8_t *bgr, const uint8_t *r8, uint8_t *refl_out,
                                  uint8_t *shading_out, int n, const int *heights, const int *widths,
                                  const unsigned long long *k_refl, const unsigned long long *k_shading,
                                  const double *srgb_steps, void *workspace, size_t workspace_bytes,
                                  void *stream);

/*
 * CV_32F variants of the two filters (never reached by the reference's CLIs, whose images come
 * from cv2.imread as uint8; provided so that callers which stop quantising between stages keep
 * the cv2.ximgproc semantics).  Same layouts as the 8-bit entry points with float pixels.
 *   rf_jbf_f32: jointBilateralFilter_32f - colour weight interpolated in a table of 4096 bins per
 *     joint channel over the joint's value range, built on the host with libm's exp: the range
 *     comes back to the host, so THIS ENTRY POINT SYNCHRONISES THE STREAM, and rf_jbf_f32 is refused
 *     (RF_E_UNSUPPORTED) on a stream that is being captured into a graph, before its tables are
 *     looked up and before anything is enqueued (rf_gf_f32 below can be captured).  A constant joint
 *     image returns RF_E_UNSUPPORTED (OpenCV switches to a Gaussian blur there), and so does
 *     BORDER_CONSTANT (its zero padding indexes OpenCV's table out of bounds).
 *   rf_gf_f32: guidedFilter on float guide/src, float result (no rounding), `iterations` chained.
 *   Both workspaces: device scratch of at least the size query's bytes, 16-byte aligned (not checked:
 *   rf_jbf_f32 keeps 32-bit range words and its float tables there, rf_gf_f32 double row sums and
 *   float planes, laid out from the workspace's start).
 */
size_t rf_jbf_f32_workspace_bytes(int n, int joint_cn);
int rf_jbf_f32(const float *joint, const float *src, float *dst, int n, int h, int w, int joint_cn,
               int src_cn, int d, double sigma_color, double sigma_space, int border,
               void *workspace, size_t workspace_bytes, void *stream);
size_t rf_gf_f32_workspace_bytes(int n, int h, int w, int guide_cn, int src_cn, int radius);
int rf_gf_f32(const float *guide, const float *src, float *dst, int n, int h, int w, int guide_cn,
              int src_cn, int radius, double eps, int iterations, void *workspace,
              size_t workspace_bytes, void *stream);

/*
 * WHDR (weighted human disagreement rate, Bell et al. 2014) of a batch of reflectance predictions.
 * Replaces the per-comparison Python loop  whdr(reflectance, comparisons, delta)  of
 * /root/reference/training/layers/whdr_layer.py:253-287 (lightness: :180-196).
 *   refl     n*c*h*w float32 device, planar [n][c][h][w], c in {1,3}
 *   points   total*5 int32 device: x1, y1, x2, y2 (pixels, inside the image), darker (0 'E', 1, 2)
 *   weights  total float64 device: darker_score of each comparison
 *   offsets  n+1 int32 device: comparisons of image i are [offsets[i], offsets[i+1])
 *   out      n float64 device: error_sum / weight_sum (0 for an image without comparisons)
 * Lightness and ratios are float32 and compared with (float)(1 + delta); the two sums are float64,
 * accumulated in comparison order.
 */
int rf_whdr_f32(const float *refl, int n, int c, int h, int w, const int *points,
                const double *weights, const int *offsets, double delta, double *out, void *stream);

/*
 * Joint bilateral filter, 8-bit, evaluated at listed pixels only, for many parameter sets in one
 * call: the bilateral half of a WHDR parameter sweep (the reference's filter_reflectance.py:1
 * "Go through color and spatial parameters and evaluate filter").
 *   joint, src, n, h, w, joint_cn, src_cn, d, border  as for rf_jbf_u8
 *   points         total_points*2 int32 device: x, y of each point (inside its image)
 *   point_offsets  n+1 int32 device: the points of image i are [point_offsets[i], point_offsets[i+1])
 *   sigma_color, sigma_space  n_params doubles each, HOST memory: parameter set p is
 *                  (sigma_color[p], sigma_space[p]); sets may differ in sigma_space, i.e. in radius
 *   out            n_params*total_points*src_cn uint8 device, must not overlap an input
 *   workspace      device scratch of at least rf_jbf_points_workspace_bytes(n_params, sigma_space,
 *                  d, joint_cn, flags) bytes (0 there = arguments the call refuses), 16-byte aligned
 *                  (not checked: chunk records, 8-byte taps and float tables, each part at a multiple
 *                  of 256 bytes from its start)
 * out[p][k][c] is, byte for byte, what rf_jbf_u8(joint, src, ..., d, sigma_color[p],
 * sigma_space[p], border, flags) writes at pixel points[k] of its image: the same radius rule,
 * sigma <= 0 rule and refusals, the same per-pixel arithmetic (taps in row-major disk order,
 * w = sw * lut[sad], separately rounded multiply and add, sum * (1/wsum) or, with
 * RF_JBF_TRUE_DIVISION, sum / wsum) and the same RF_JBF_GREY_AS_BGR rule; RF_JBF_FORCE_GENERIC is
 * accepted and changes nothing, any other flag bit is refused (RF_E_BADARG).  Points are not
 * read on the host, so they cannot be checked: a point outside its image gives unspecified bytes
 * (the kernel clamps it and never reads outside the images).  The parameter tables are built on
 * the host by the code rf_jbf_u8 uses and staged in the workspace; rf_jbf_u8's table cache is
 * left alone.  THIS ENTRY POINT SYNCHRONISES THE STREAM (before its launch, to upload the tables)
 * and is refused (RF_E_UNSUPPORTED) on a stream that is being captured into a graph.
 */
size_t rf_jbf_points_workspace_bytes(int n_params, const double *sigma_space, int d, int joint_cn,
                                     int flags);
int rf_jbf_points_u8(const uint8_t *joint, const uint8_t *src, int n, int h, int w, int joint_cn,
                     int src_cn, const int *points, const int *point_offsets, int total_points,
                     int n_params, const double *sigma_color, const double *sigma_space, int d,
                     int border, int flags, uint8_t *out, void *workspace, size_t workspace_bytes,
                     void *stream);

/*
 * rf_jbf_points_u8 over images of different sizes (IIW photos come in many shapes): one call, one
 * launch, whatever the sizes are.
 *   joint, src     the n images tightly packed one after another: image i starts at pixel
 *                  sum over j < i of heights[j] * widths[j] (offsets are formed in 64 bits) and is
 *                  heights[i] rows of widths[i] pixels
 *   heights, widths  n ints each, HOST memory (like the sigmas): every entry must be > 0
 *   workspace      device scratch of at least rf_jbf_points_ragged_workspace_bytes(n, n_params,
 *                  sigma_space, d, joint_cn, flags) bytes: rf_jbf_points_workspace_bytes of the same
 *                  arguments plus one 256-byte-aligned block of 16 * n bytes (a record of first
 *                  pixel, height and width per image, staged with the tables in the call's one copy);
 *                  0 = arguments the call refuses; 16-byte aligned like rf_jbf_points_u8's
 * Everything else is rf_jbf_points_u8's contract: out[p][k][c] is, byte for byte, what rf_jbf_u8 on
 * image i alone (n = 1, heights[i], widths[i]) writes at pixel points[k]; the same radius, sigma,
 * flag and border rules and refusals; out must not overlap an input (judged on the summed pixel
 * count); n == 0 is RF_OK, total_points == 0 is RF_OK after the checks.  A point outside its image
 * is clamped to that image's own size (unspecified bytes, never a read outside the buffers).
 * The lanes run the code of rf_jbf_points_u8's kernel and the launch plan is the same function of
 * total_points.  SYNCHRONISES THE STREAM once, and is refused on a capturing stream.
 */
size_t rf_jbf_points_ragged_workspace_bytes(int n, int n_params, const double *sigma_space, int d,
                                            int joint_cn, int flags);
int rf_jbf_points_ragged_u8(const uint8_t *joint, const uint8_t *src, int n, const int *heights,
                            const int *widths, int joint_cn, int src_cn, const int *points,
                            const int *point_offsets, int total_points, int n_params,
                            const double *sigma_color, const double *sigma_space, int d, int border,
                            int flags, uint8_t *out, void *workspace, size_t workspace_bytes,
                            void *stream);

/*
 * WHDR of uint8 predictions sampled at judgement points (rf_jbf_points_u8's output, or whole
 * images taken as point lists).
 *   samples        n_sets*set_stride*c uint8 device: pixel q of set s is at (s*set_stride + q)*c
 *   point_offsets  n int32 device (the n+1 array of rf_jbf_points_u8 serves): the points of image i
 *                  are the pixels point_offsets[i] + index of each set
 *   comps          total*3 int32 device: index of point 1, index of point 2 (into image i's
 *                  points), darker (0 'E', 1, 2)
 *   weights        total float64 device; comp_offsets n+1 int32 device (as in rf_whdr_f32)
 *   out            n_sets*n float64 device: out[s*n + i] = WHDR of image i in set s
 * Each byte becomes (float)byte / 255.0f (correctly rounded), and from there on the lightness,
 * decision and float64 sums are rf_whdr_f32's: the result equals rf_whdr_f32 on the planar float
 * images bytes / 255.0f.  Indices are not checked (device data); a read never leaves the set.
 */
int rf_whdr_points_u8(const uint8_t *samples, int n_sets, long long set_stride, int c, int n,
                      const int *point_offsets, const int *comps, const double *weights,
                      const int *comp_offsets, double delta, double *out, void *stream);

/*
 * PNG encode on the device: n packed 8-bit images of different sizes to one complete zlib stream
 * per image - the body of a PNG file's single IDAT chunk; the caller adds signature, IHDR, the
 * chunk framing and IEND.
 *   images         the n images tightly packed one after another (as for rf_jbf_ragged_u8), cn_in
 *                  channels each: 1 (written as colour type 0), 3 (BGR in memory, written as colour
 *                  type 2 in RGB order), or 1 with RF_PNG_GREY_AS_RGB (colour type 2, three equal
 *                  bytes per pixel, without a replicated copy)
 *   heights, widths  n ints each, HOST memory, every entry > 0
 *   streams        device buffer of stream_capacity >= rf_png_stream_bound(...) bytes; must not
 *                  overlap images.  The stream of image i is the bytes
 *                  [stream_offsets[i], stream_offsets[i + 1]) of it: the streams lie one after
 *                  another without gaps, so stream_offsets[n] bytes are used
 *   stream_offsets n + 1 uint64, DEVICE memory, written by the call
 *   workspace      device scratch of at least rf_png_workspace_bytes(...) bytes, 16-byte aligned
 * The raw stream of an image is, per row, the filter byte 2 (Up) and the differences to the row
 * above (zeros above the first row), cut into chunks of one library-wide length (rf_debug_png_plan)
 * that are deflated independently: literals and runs of the previous byte (length 3..258 at distance
 * 1) in one dynamic-Huffman block per chunk, closed by an empty stored block so that chunks join on
 * byte boundaries, or one stored block where that is shorter.  The stream is 78 01, the chunks,
 * 03 00 and the Adler-32 of the raw stream; any inflate reads it.  Its bytes are a function of the
 * input alone (the same on every run), and differ from zlib's for the same pixels.
 * rf_png_stream_bound: sum over the images of 2 + sum over its chunks of (chunk bytes + 9) + 2 + 4;
 * an image whose own bound reaches 2^31 is refused (one IDAT chunk holds 2^31 - 1 bytes).  Both size
 * queries return 0 for n <= 0 and for arguments the call refuses.  n == 0 is RF_OK and touches
 * nothing.  Three launches per call whatever the list holds.  SYNCHRONISES THE STREAM once (before
 * its launches, to upload the image table) and is refused (RF_E_UNSUPPORTED) on a capturing stream.
 */
#define RF_PNG_GREY_AS_RGB 1 /* cn_in = 1 only: write three equal samples per pixel */
size_t rf_png_stream_bound(int n, const int *heights, const int *widths, int cn_in, int flags);
size_t rf_png_workspace_bytes(int n, const int *heights, const int *widths, int cn_in, int flags);
int rf_png_deflate_ragged_u8(const uint8_t *images, int n, const int *heights, const int *widths,
                             int cn_in, int flags, uint8_t *streams, size_t stream_capacity,
                             unsigned long long *stream_offsets, void *workspace,
                             size_t workspace_bytes, void *stream);

/*
 * The device half of a PNG decode: the inflated IDAT streams of n images of different sizes and
 * formats to packed 8-bit BGR images (what cv2.imread returns), plus one flag byte per image.  The
 * caller parses the files and inflates them (one serial zlib stream per file: host work); the entry
 * undoes the row filters and unpacks the samples.
 *   raw            device buffer holding the inflated streams: for image i the bytes
 *                  [raw_offsets[i], raw_offsets[i + 1]), h rows of one filter byte and w * bpp
 *                  filtered bytes.  OVERWRITTEN: the rows are reconstructed in place
 *   raw_offsets    n + 1 uint64, HOST memory; raw_offsets[i + 1] - raw_offsets[i] must equal
 *                  h * (1 + w * bpp)
 *   heights, widths, formats  n ints each, HOST memory.  formats[i] = RF_PNG_FORMAT(bit depth,
 *                  colour type): depth 8 or 16 with colour type 0 (grey), 2 (RGB), 4 (grey + alpha),
 *                  6 (RGBA), or depth 8 with colour type 3 (palette); bpp = 1, 2, 3, 4, 6 or 8.  No
 *                  interlace
 *   palettes       device, 768 bytes per image (256 RGB entries, unused ones zero), read for the
 *                  images of colour type 3 only; may be NULL where the list holds none
 *   images         device, written: the n images tightly packed one after another, 3 bytes per
 *                  pixel in BGR order (grey replicated, alpha dropped, the high byte of a 16-bit
 *                  sample, the palette entry of an index); must not overlap raw
 *   image_flags    device, n bytes, written: RF_PNG_FLAG_GREY where the three channels are equal at
 *                  every pixel of the image, RF_PNG_FLAG_BAD_FILTER where a row's filter byte is
 *                  above 4 (such a row is taken as filter 0; the call still returns RF_OK)
 *   workspace      device scratch of at least rf_png_unfilter_workspace_bytes(...) bytes (48 + 4
 *                  bytes per image, each part rounded up to 256), 16-byte aligned
 * Refused before any device work: NULL pointers, n < 0, a size <= 0, an unsupported format
 * (RF_E_UNSUPPORTED), a raw length that does not match, an image whose raw stream or pixel count
 * reaches 2^31 (RF_E_UNSUPPORTED), a short (RF_E_WORKSPACE) or misaligned workspace, images
 * overlapping raw.  The size query returns 0 for n <= 0 and for arguments the call refuses.  n == 0
 * is RF_OK and touches nothing.  The bytes written are a function of the input alone.  Three
 * launches per call whatever the list holds.  SYNCHRONISES THE STREAM once (before its launches, to
 * upload the image table) and is refused (RF_E_UNSUPPORTED) on a capturing stream.
 */
#define RF_PNG_FORMAT(depth, ctype) (((depth) << 8) | (ctype))
#define RF_PNG_FLAG_GREY 1       /* image_flags: all three channels equal at every pixel */
#define RF_PNG_FLAG_BAD_FILTER 2 /* image_flags: a filter byte above 4 was seen */
size_t rf_png_unfilter_workspace_bytes(int n, const int *heights, const int *widths,
                                       const int *formats);
int rf_png_unfilter_ragged_u8(uint8_t *raw, const unsigned long long *raw_offsets, int n,
                              const int *heights, const int *widths, const int *formats,
                              const uint8_t *palettes, uint8_t *images, uint8_t *image_flags,
                              void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* REFLECTANCE_FILTERING_H */
