/*
 * reflectance_filtering_debug.h -- test and benchmark switches of librf_hip.so.
 *
 * NOT part of the drop-in boundary (include/reflectance_filtering.h): nothing here is needed
 * to replace the reference's native calls.  The switches select alternative kernels that the
 * parity tests and the timing tools compare against the default ones; they are process-global,
 * not meant to be flipped while other threads are inside the library, and all default to 0.
 *
 *   "gf_two_kernel"      guided filter: row-sum / column-sum kernel pair for every radius (the
 *                        default fuses stage 2 for every radius 1..128); identical bytes
 *   "jbf_compiler_loop"  joint bilateral: compiler-scheduled tap loop; identical bytes.  (This switch,
 *                        "jbf_lookahead1" and "jbf_stage_only" act on the 64x64-tile kernel, radius <= 52;
 *                        the slab kernel of radius 53..468 has one tap loop and ignores them - its
 *                        independent check is RF_JBF_FORCE_GENERIC, tests/test_gpu_parity.py)
 *   "jbf_tile64_only"    joint bilateral: no strip tiles at the image remainder; identical bytes
 *   "jbf_tune"           joint bilateral: kernel-variant override 1..7 (tools/jbf_tune.py)
 *   "jbf_f32_untiled"    float joint bilateral: one-thread-per-pixel kernel; identical values
 *   "cnn_lds_columns"    CNN: activations pass between layers through LDS columns instead of
 *                        registers; identical values
 *   "gf_seg_rows"        guided filter: rows per stage-1 segment (tools/gf_seg_sweep.py); 0 =
 *                        chosen by the library; identical bytes
 *   "gf_one_stream"      guided filter: the whole batch on the caller's stream (the default runs
 *                        the two halves of a batch on the caller's stream and on a side stream of
 *                        the library, forked / joined with events inside the call); identical bytes
 *   "gf_force_two_streams"  guided filter: fork the side stream for every chunk of two or more
 *                        images (the default decides by batch size and src kind); identical bytes
 *   "gf_guide_cache"     guided filter, experiment: an iterated call keeps the guide's window
 *                        statistics of its first pass in the workspace (36 B per pixel) and later
 *                        passes box-sum only the src quantities; identical bytes, measured slower
 *                        (profiles/r03_gf_guide_cache.md), off by default
 *   "gf_chained"         guided filter, radius 45 / 52: the column walk without a row-walk kernel
 *                        (every 16-column block takes its row sums from its left neighbour through
 *                        tagged slots); identical bytes, measured slower
 *                        (profiles/r04_gf_chained.md), off by default
 *   "gf_no_compact"      guided filter: grey images of a 3-channel src are read and handed from pass
 *                        to pass as three channels (the default keeps them as one byte per pixel in
 *                        the workspace); identical bytes
 *   "jbf_stage_only"     joint bilateral: stage the tile and return WITHOUT WRITING dst
 *                        (tools/jbf_tune.py --stage-only, timing only)
 *   "gf_exp_skip"        guided filter, TIMING ONLY, WRONG RESULTS: bit 0 no stage 1, bit 1 no row
 *                        walk, bit 2 no column walk (tools/gf_c5_exp.py)
 *   "jbf_lookahead1"     joint bilateral: the grey asm tap loop with its LUT gathers one column step
 *                        ahead of their use and a full wait per step (the round-4 form; the default keeps
 *                        them two steps ahead, four gathers in flight across a step); identical bytes
 *   "gf_stagger"         guided filter: staggered two-stream schedule - the stage-1 launches of the
 *                        parts of a chunk are chained by events in (pass, part) order, parts alternating
 *                        between the caller's stream and the side stream, so that one part's stage 1
 *                        always faces the other's walks; identical bytes, measured no faster than the
 *                        default (profiles/r05_c5_overlap.md), off by default
 *   "gf_parts"           ... parts per chunk in that schedule (even, 2..16; 0 = 2)
 *   "gf_s1_cap"          guided filter: stage-1 workgroups per CU (1..3, by a dynamic-LDS pad; 0 =
 *                        whatever fits); identical bytes
 *   "gf_s1_min_wgs"      guided filter: workgroups a stage-1 launch should at least have (chooses the
 *                        rows per segment; 0 = chosen by the library); identical bytes
 *   "gf_s1_legacy_strips"  guided filter: stage-1 strips with a halo of exactly r columns on either side
 *                        (rounds 1-5; the default aligns halo and width to 16 columns and takes a whole
 *                        wave of halo where that costs no strip); identical bytes
 *   "gf_exact"           guided filter, radius 45 / 52, width a multiple of 16: exact-row stage 2 - rows
 *                        whose alpha / beta pass an exactness test take no sequential row walk (block sums
 *                        from stage 1, the rest listed and walked); identical bytes, measured slower
 *                        (profiles/r06_gf_exact.md), off by default
 *   "gf_exact_all_flagged"  ... with every row treated as failing the test (exercises the list path)
 *   "gf_cw_chan_run"     guided filter, colour src, passes of an iterated call that hand their result on as
 *                        planes: n + 1 = the column walk takes an XCD's (block, channel) items in runs of n
 *                        blocks per channel (0 = the library's choice, 64; 1 = channel fastest); identical bytes
 *   "jbf_no_msad"        joint bilateral, 3-channel joint: every wave runs the asm tap loop that masks the
 *                        src byte out of the tap texel (v_and_b32 + v_sad_u8).  By default a wave none of
 *                        whose centre pixels has a zero joint channel runs the masked-SAD form (v_msad_u8 on
 *                        the unmasked texel, one VALU instruction per step less) and only the other waves
 *                        this one; identical bytes.  There is no switch the other way round: the
 *                        masked-SAD form is wrong for a centre with a zero channel.  The masked-SAD form
 *                        exists for the default grey loop (gathers two steps ahead) and the colour loop, in
 *                        the tile and the slab kernel; under "jbf_lookahead1" (the round-4 grey loop) and
 *                        "jbf_compiler_loop" every wave keeps the mask, whatever this option says.
 *   "jbf_no_two_wg"      joint bilateral, radius <= 36: grey tiles run in jbf_tile64_kernel at one workgroup
 *                        per CU, as colour tiles do, in one launch (the default: the grey map - a clearing
 *                        launch and one pass over the images - writes one byte per tile, jbf_tile64_kernel
 *                        filters the tiles flagged as colour, and jbf_tile64x2_kernel the grey ones at two
 *                        workgroups per CU - four launches, three with a single-channel src, one where both
 *                        buffers have one channel); identical bytes
 *   "jbf_vote_scan"      joint bilateral, two-per-CU route: the tile bytes come from one launch of
 *                        jbf_tile64x2_kernel in which every tile scans its own region, tile and halo (the
 *                        form before the grey map, which reads every texel 4.6 times at radius 33; a call
 *                        with a WRAP border takes it without the switch); identical tile bytes, identical bytes
 *   "jbf_no_dead_skip"   joint bilateral, two-per-CU route: the waves of a tile whose four rows all lie
 *                        below the image walk the tap loop like the others (the default: they stage, meet
 *                        the barriers and skip the loop); identical bytes
 *   "colorize_chunk_px"  ragged colourise (rf_colorize_ragged_srgb_u8): pixels per workgroup chunk, a
 *                        multiple of 256 that replaces the plan rule (0 = the rule; anything else is
 *                        refused with RF_E_BADARG by the entry and the plan query); identical bytes.
 *                        Lets a test with tiny images run many chunks per image and chunks of more
 *                        than 2048 pixels, and tools/decompose_list_time.py time other chunk lengths.
 *
 * The grey-guide form of the guided filter (rf_gf_ex_u8 with RF_GF_GREY_AS_BGR) has no stage 1 for
 * "gf_guide_cache" and "gf_exact": while either is set, such a call returns RF_E_UNSUPPORTED.  Every
 * other switch above applies to it as to a colour guide.
 *
 * Besides the switches, rf_debug_jbf_points_plan reports the launch plan of rf_jbf_points_u8 (how
 * its parameter sets are cut into chunks and how many points a wave of each chunk takes) without
 * touching a device, so that tests can assert which lane mapping a call runs at, and
 * rf_debug_jbf_ragged_plan the tile classes rf_jbf_ragged_u8 launches, rf_debug_jbf_ragged_slab_plan
 * its one launch of tap-row slabs at radius 53..468, rf_debug_colorize_ragged_plan the chunk
 * length and grid of rf_colorize_ragged_srgb_u8, and rf_debug_gf_ragged_plan the route and grids of
 * rf_gf_ragged_u8.
 */
#ifndef REFLECTANCE_FILTERING_DEBUG_H
#define REFLECTANCE_FILTERING_DEBUG_H

#ifdef __cplusplus
extern "C" {
#endif

/* Sets option `name` to `value` (>= 0) and returns its previous value; RF_E_BADARG (-1) for an
 * unknown name. */
int rf_debug_option(const char *name, int value);

/* Measurement aid of bench.py: one wave on `stream` brackets `micros` microseconds of wall time
 * (s_memrealtime, 100 MHz) with the shader-cycle counter (s_memtime), sleeping in between, and
 * writes {shader cycles, 100 MHz ticks} to the two device words at out2.  Launched on a second
 * stream beside a running kernel it reads the clock the chip holds under that kernel's load:
 * MHz = 100 * out2[0] / out2[1]. */
int rf_debug_clock_probe(unsigned long long *out2, int micros, void *stream);

/* The toolchain this library was compiled with (`hipcc --version`, first two lines): the inline-asm
 * hazard audit of tests/test_cabi.py holds for the machine code of that compiler. */
const char *rf_debug_build_info(void);

/* The launch plan of rf_jbf_points_u8(n_params sets with these sigma_space, d, joint_cn, flags) for
 * a call of total_points points: per chunk, in launch order (decreasing radius; the sets of one
 * sigma_space, after the `<= 0 -> 1` rule, in chunks of at most 64), the four ints
 * {radius, nsets, ppw, waves} - ppw = points a wave takes, waves = ceil(total_points / ppw) - for the
 * first max_chunks chunks at out[4 * chunk].  Decided by the code the entry launches from.  Returns
 * the number of chunks of the call (it may exceed max_chunks; out may be NULL when max_chunks is 0),
 * or a negative RF_E* for arguments the entry refuses.  Host only: needs no device. */
int rf_debug_jbf_points_plan(int n_params, const double *sigma_space, int d, int joint_cn, int flags,
                             int total_points, int *out, int max_chunks);

/* The launches of rf_jbf_ragged_u8 for these arguments: per tile class, in launch order (64x64
 * tiles, the 32x128 and 16x256 bottom strips, the 128x32 right strip; classes without tiles are
 * left out), the four ints {tile rows, tile columns, row pitch, tiles of all images} for the first
 * `cap` launches at out[4 * launch].  Decided by the planning function the entry launches from (the
 * debug switches included; the LDS probe of the device is not consulted).  Returns the number of
 * launches (it may exceed cap; out may be NULL when cap is 0), -1 where the entry falls back to
 * rf_jbf_u8 once per image, or the entry's RF_E_UNSUPPORTED (-2) for channels or a radius it
 * refuses.  RF_E_BADARG (bad sizes, NULL size arrays, unknown flag bits, a bad cap) is -1 as well:
 * for n > 0 and a valid cap, rf_jbf_ragged_workspace_bytes of the same arguments is 0 exactly when
 * the entry refuses them, which tells the two apart.  Host only: needs no device. */
int rf_debug_jbf_ragged_plan(int n, const int *heights, const int *widths, int joint_cn, int src_cn,
                             int d, double sigma_color, double sigma_space, int flags, int *out,
                             int cap);

/* The slab launch of rf_jbf_ragged_u8 (radius 53..468, where no tile class of the query above holds
 * the radius: every image's 64x64 tiles in one launch of the slab kernel) for the same arguments:
 * the seven ints {row pitch, LUT replicas, rows per band and rows per slab with 4-byte texels, the
 * same two with 6-byte texels (0, 0: a colour tile takes one grey pass per channel; always 0, 0 for
 * a single-channel src), 64x64 tiles of all images} at out[0..6] when cap >= 1.  Decided by the
 * functions the entry and rf_jbf_u8 launch from (the debug switches included; the LDS probe of the
 * device is not consulted).  Returns 1 where the entry runs that launch (out may be NULL when cap
 * is 0), -1 where it does not (the tile classes above, or rf_jbf_u8 once per image), and what
 * rf_debug_jbf_ragged_plan returns for arguments the entry refuses or a bad cap - told apart from
 * the -1 above in the same way.  Host only: needs no device. */
int rf_debug_jbf_ragged_slab_plan(int n, const int *heights, const int *widths, int joint_cn,
                                  int src_cn, int d, double sigma_color, double sigma_space, int flags,
                                  int *out, int cap);

/* The route of rf_jbf_u8's grey tiles for a call of n images of h x w: the four ints {two-per-CU
 * route taken (1 / 0), tile rows resident in the LDS (64 output rows + a slab's halo; 0 off the route),
 * 64x64 tiles of the route's launches, bytes of the library's tile-flag buffer the call needs (one
 * byte per tile, a power of two of at least 4 KiB; 0 where both buffers have one channel: no bytes, one
 * launch)} at out[0..3].  The resident rows are a slab window, not a ring: the tile is staged again for
 * every slab.  Decided by the functions the entry launches from (the debug switches included); what the
 * query cannot see - the LDS probes of the device, a capturing stream whose flag buffer would have to
 * grow, more than 16 streams holding a buffer - sends a call down the one-per-CU path all the same:
 * rf_debug_jbf_two_wg_calls counts the calls that really launched the route.
 * Returns 1 on the route, 0 off it, or the entry's refusal code.  Host only: needs no device. */
int rf_debug_jbf_two_wg_plan(int n, int h, int w, int joint_cn, int src_cn, int d, double sigma_color,
                             double sigma_space, int flags, int *out);

/* The number of rf_jbf_u8 calls of this process so far that launched the two-per-CU route (the grey map
 * that writes the tile bytes where a buffer has three channels - or, under "jbf_vote_scan", the scan
 * launch -, jbf_tile64_kernel on the flagged tiles of a 3-channel src, jbf_tile64x2_kernel on the grey
 * tiles), modulo 2^31.  A test that means to exercise the route asserts that the count moved. */
int rf_debug_jbf_two_wg_calls(void);

/* The tile bytes of the two-per-CU route as the last call on `stream` (on the current device) left them:
 * copies min(cap, size of the stream's tile-flag buffer) bytes to the HOST array out and returns that
 * number, 0 where the stream holds no buffer.  Byte t belongs to tile t of the route's launches (image
 * by image, row by row of the main area's 64x64 tiles): bit 0 = the src is not grey somewhere in the
 * tile's region (tile and halo as staged, through the border rule), bit 1 = the joint is grey
 * everywhere in it; bytes beyond the last call's tiles are whatever earlier calls left.  SYNCHRONISES
 * the stream and cannot be captured into a graph (RF_E_UNSUPPORTED on a capturing stream). */
int rf_debug_jbf_tile_flags(void *stream, unsigned char *out, int cap);

/* The launch plan of rf_colorize_ragged_srgb_u8 for images of these sizes: the ints {chunk_px,
 * workgroups} - the pixels one workgroup takes and the grid of the histogram and write kernels -
 * followed by each image's first workgroup (the running sum of ceil(h * w / chunk_px)), as many of
 * these 2 + n ints as `cap` holds, at out.  Decided by the planning function the entry launches from
 * (the "colorize_chunk_px" switch included).  Returns n (out may be NULL when cap is 0), or the
 * entry's refusal code for sizes it refuses or a bad cap.  Host only: needs no device. */
int rf_debug_colorize_ragged_plan(int n, const int *heights, const int *widths, int *out, int cap);

/* The route of rf_gf_ragged_u8 for these arguments and, on the ragged route, its launches: the six
 * ints {launches per pass (3), workgroups of stage 1, of the row walk, of the column walk, left halo
 * and output columns of a stage-1 strip}, as many of them as `cap` holds, at out.  Decided by the
 * planning function the entry launches from (the debug switches included).  Returns 1 on the ragged
 * route, 0 where the entry calls rf_gf_ex_u8 once per image (and for n == 0; out is left alone), or the
 * entry's refusal code for arguments it refuses or a bad cap.  Host only: needs no device. */
int rf_debug_gf_ragged_plan(int n, const int *heights, const int *widths, int guide_cn, int src_cn,
                            int radius, int flags, int *out, int cap);

/* The images rf_gf_u8, rf_gf_ex_u8 (float_kernels = 0: radius <= 128; 1: beyond) and rf_gf_f32
 * (float_kernels = 1) run at once where the workspace has room for `chunk` images of h x w: at most 16383
 * (float kernels: 65535), and no more than the launches that fold the chunk into gridDim.x take (fewer
 * than 2^32 work-items each).  0: one such image is too large for a launch, and the entries refuse it
 * (RF_E_UNSUPPORTED).  Decided by the function the entries take their chunk from.  Host only. */
int rf_debug_gf_launch_chunk(int chunk, int h, int w, int src_cn, int float_kernels);

/* The plan of rf_png_deflate_ragged_u8 for images of these sizes: the ints {chunk length in raw
 * bytes (one library-wide constant), chunks of all images} followed by each image's number of chunks
 * (ceil(h * (1 + w * c_out) / chunk length)), as many of these 2 + n ints as `cap` holds, at out.
 * Returns n (out may be NULL when cap is 0; n == 0 gives the two leading ints), or the entry's
 * refusal code for arguments it refuses or a bad cap.  Host only: needs no device. */
int rf_debug_png_plan(int n, const int *heights, const int *widths, int cn_in, int flags, int *out,
                      int cap);

#ifdef __cplusplus
}
#endif
#endif /* REFLECTANCE_FILTERING_DEBUG_H */
