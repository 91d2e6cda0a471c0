/*
 * hipcanny.h -- C ABI of libhipcanny.so: the MI355X (gfx950) Canny edge detector that replaces
 * the CUDA hot path of axoloto/CudaCam (class cvp::cuda::CannyEdge).
 *
 * Every entry point cites the reference interface it replaces (paths relative to the CudaCam
 * tree).  The C++ drop-in classes in include/cvp/ (cvp::cvPipeline, cvp::cuda::CannyEdge) and the
 * Python binding in cudacam_amd/ are thin layers over exactly these functions.  No torch / HIP
 * types appear in the signatures: device pointers and streams travel as void*.
 *
 * Threading: one context = one device + one stream; a context is not thread-safe, different
 * contexts may be used from different threads (reference: single-threaded, default stream,
 * src/imgui/imguiApp.cpp:496-522).
 * Errors: 0 = ok, negative = failure (see HC_E_*); hc_last_error() returns a message.  The
 * reference logs and exits the process instead (src/cvp/helper.hpp:4-17).
 */
#ifndef HIPCANNY_H
#define HIPCANNY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hc_ctx hc_ctx;

/* Stage ids: cvp::CannyStage, src/cvp/define.hpp:9-17 */
enum { HC_STAGE_MONO = 0, HC_STAGE_GAUSSIAN = 1, HC_STAGE_GRADIENT = 2, HC_STAGE_NMS = 3, HC_STAGE_THRESH = 4, HC_STAGE_HYSTER = 5 };

/* Parity modes.  R: bit-exact with the reference kernels (src/cvp/cannyEdgeD.cu).
 * O: cv::Canny(img, low, high, apertureSize, L2gradient) semantics (no blur, replicate border; apertureSize 3 unless
 *    HC_OPT_APERTURE is 5; L2gradient false unless HC_OPT_L2_GRADIENT is set), and cv::Canny(dx, dy, edges, low, high,
 *    L2gradient) through hc_run_gradients_device.  Restated from the published algorithm (tests/ and oracle/); not
 *    pinned against a build of OpenCV itself. */
enum { HC_MODE_R = 0, HC_MODE_O = 1 };

enum {
  HC_OK = 0,
  HC_E_ARG = -1,      /* bad argument (null, size/channel mismatch, unsupported type) */
  HC_E_HIP = -2,      /* a HIP runtime call failed (hc_last_error() has the hipError string) */
  HC_E_STATE = -3,    /* call sequence error (e.g. run before upload) */
  HC_E_NOGPU = -4     /* no usable gfx950 device */
};

/* Replaces CannyEdge::CannyEdge + _initAlloc (src/cvp/cannyEdgeH.cu:16-38, 340-385).
 * width/height/channels as in the reference constructor; max_batch frames can be resident and
 * processed per hc_run (the reference is single-frame: max_batch = 1).  Defaults follow
 * cannyEdgeH.cu:22-24: low = 10, high = 40 (Mode O: 50/150).  Returns NULL on failure. */
hc_ctx *hc_create(int device, int width, int height, int channels, int max_batch, int mode);

/* Replaces CannyEdge::~CannyEdge + _endAlloc (cannyEdgeH.cu:40-47, 387-407). */
void hc_destroy(hc_ctx *ctx);

/* Replaces setLowThreshold/setHighThreshold (src/cvp/cannyEdgeH.hpp:25-29): the pair is stored as
 * given after clamping to 0..255 (Mode R) and ordering low <= high. */
int hc_set_thresholds(hc_ctx *ctx, int low, int high);
int hc_get_thresholds(const hc_ctx *ctx, int *low, int *high);

/* Mode O: thresholds per frame for the runs that follow (hc_run, hc_run_device, hc_run_gradients_device): frame f of a run
 * is cut with d_thr[2f], d_thr[2f+1] exactly as if hc_set_thresholds(d_thr[2f], d_thr[2f+1]) had preceded a run of that
 * frame alone.  d_thr: device memory, int32 [nframes][2], 4-byte aligned, caller-owned; it is read by the run's front
 * kernel on the context stream (plain and pipelined mode alike), so work queued on that stream before the run may
 * write it and work queued after the run may overwrite it -- no host synchronisation.  NULL: back to the context's pair.
 * Each pair is normalised on the device as hc_set_thresholds does it on the host: clamped to 0..32767, swapped if
 * low > high, squared under HC_OPT_L2_GRADIENT (frame_threshold_pair, cudacam_amd/csrc/canny_params.h).  Kernels: k_front_o,
 * k_front8o and k_front_o_ext at HC_OPT_APERTURE 5 and on given gradients each have an instantiation that reads the table, which
 * the launcher picks when one is installed; runs without a table execute the code they did before the table existed.  Forms
 * and work split are the same either way.
 * HC_E_ARG: a mode R context (its thresholds are the reference's u8 sliders through the wrap bands; per-frame thresholds
 * for mode R are not offered); a pointer that is not 4-byte aligned; nframes outside 1..max_batch; and, from the run
 * itself, a run of more frames than the table holds.
 * hc_canny_device keeps its per-call thresholds and ignores the table; it leaves the table installed, as it leaves the
 * context's settings untouched.  The table changes nothing else: hc_get_thresholds still reports the context's pair; the
 * hysteresis schedule and history, hc_last_run_info, the stage timers, HC_OPT_DEBUG_TAPS and the staging of views are as
 * without it; the provisional map of pipelined k_front8o runs uses the frame's own `high`. */
int hc_frame_thresholds_device(hc_ctx *ctx, const void *d_thr, int nframes);

/* Replaces _loadInputImage (cannyEdgeH.cu:122-152): host frames -> device.  row_stride = cv::Mat::step,
 * frame_stride = bytes between consecutive frames.  Asynchronous on the context stream when the
 * host memory is pinned. */
int hc_upload(hc_ctx *ctx, const uint8_t *host, size_t row_stride, size_t frame_stride, int nframes);

/* Replaces CannyEdge::run's stage switch (cannyEdgeH.cu:49-120) for the frames last uploaded:
 * runs the pipeline up to final_stage and leaves that stage's u8 image in the output buffer
 * (what _sendOutputToOpenGL copies into the PBO, cannyEdgeH.cu:154-212).  Asynchronous. */
int hc_run(hc_ctx *ctx, int final_stage, int nframes);

/* The same on caller-owned device memory (no upload/download): `d_in` holds nframes frames of
 * width*channels bytes per row, `d_out` receives nframes tight-or-pitched u8 images.  Pointers,
 * pitches and frame strides must be multiples of 4 bytes (others are staged through internal buffers, see
 * hc_last_run_info).  Asynchronous on the context stream.
 * Readable extent: the fast kernels load whole pixel groups, so EVERY row -- the last row of the last frame
 * included -- must be readable for min(in_pitch, round_up(width, 8) * channels) bytes from its first byte: a
 * caller whose rows are padded to whole 8-pixel groups (in_pitch >= round_up(width, 8) * channels) must own that
 * padding after the last row too, i.e. allocate height * in_pitch bytes per frame.  No row is ever read beyond
 * its pitch.  What those bytes hold never changes a result: they may be row padding, the next frame, or -- for an ROI of
 * a larger image -- the neighbouring pixels of the parent.
 * Output views (this entry, hc_run_gradients_device and hc_hysteresis_device alike): only the bytes [row, row + width)
 * of each of the height rows of each frame are written -- never the rest of a pitch, the gap between frames, or anything
 * before or after the view -- in plain and in pipelined mode, in place and staged, so `d_out` may be an ROI of a larger
 * image.  The input is never written.
 * What keeps a view in place: base pointer, pitch and frame stride that are multiples of 4 (no 8- or 16-byte
 * alignment is needed, on either side; 16-byte aligned outputs merely get wider stores), and for the input of a
 * HC_STAGE_HYSTER run rows that hold whole pixel groups (above).  Anything else is staged -- one extra device-to-device
 * copy of width (x channels) bytes per row, reported by hc_last_run_info -- and gives the same bytes.
 * Views of 4 GiB and more: the front kernels address the rows of a frame with 32-bit offsets.  An input view with
 * height * in_pitch >= 2^32 is therefore staged (reported as such); an output view with height * out_pitch >= 2^32 stays
 * in place, but a pipelined run writes no provisional map into it (HC_OPT_PIPELINE below: the hysteresis then writes the
 * whole map, as it does in plain mode).  Results are the same. */
int hc_run_device(hc_ctx *ctx, const void *d_in, size_t in_pitch, size_t in_frame_stride, void *d_out, size_t out_pitch,
                  size_t out_frame_stride, int nframes, int final_stage);

/* Mode O: cv::Canny's second overload, cv::Canny(dx, dy, edges, low, high, L2gradient) (cv::cuda::CannyEdgeDetector::
 * detect(dx, dy, edges)): `d_dx` / `d_dy` hold nframes frames of caller-computed int16 derivatives (CV_16SC1, or CV_16SC3:
 * 3 interleaved channels as the context's `channels`), both with the same `pitch` and `frame_stride` in BYTES; `d_out`
 * receives the u8 edge maps as for hc_run_device.  The rest of the mode O pipeline after its Sobel runs (magnitude, the
 * 3-channel select, NMS, thresholds, hysteresis) in 32-bit two's-complement arithmetic with wrap-around, as canny.cpp's
 * `int`: for full-range input the tangent test's x * (TG22 + 2^16) wraps once |dx| >= 27146, and the L2 magnitude wraps
 * to INT_MIN for dx = dy = -32768.  Always runs to HC_STAGE_HYSTER; honours HC_OPT_L2_GRADIENT, ignores HC_OPT_APERTURE;
 * stream semantics as hc_run_device (hc_set_stream, HC_OPT_PIPELINE).  Addresses, pitch and frame stride need only be
 * even (odd widths with tight rows are fine); no byte outside [row start, row start + 2 * channels * width) of a row is
 * read.  HC_E_ARG for a mode R context, null or odd pointers / pitches, pitch < 2 * channels * width, nframes outside
 * 1..max_batch. */
int hc_run_gradients_device(hc_ctx *ctx, const void *d_dx, const void *d_dy, size_t pitch, size_t frame_stride, void *d_out,
                            size_t out_pitch, size_t out_frame_stride, int nframes);

/* Mode O: cv::Canny(img, edges, low, high, apertureSize, L2gradient) in one call on caller-owned device memory, with
 * cv::Canny's own argument list: any of its apertures -- 3, 5, 7, -1 (Scharr) -- and thresholds in cv::Canny's units.
 * `d_in` / `d_out` as for hc_run_device: u8 frames of the context's width, height and channels (1, or 3 interleaved: the
 * first channel with the largest magnitude gives a pixel's gradient), u8 edge maps out.  Always runs to HC_STAGE_HYSTER.
 * low, high, aperture and l2gradient belong to the call: they neither read nor change the context's thresholds,
 * HC_OPT_APERTURE or HC_OPT_L2_GRADIENT, and a following hc_run_device behaves as if this call had not happened.
 * Thresholds, as canny.cpp: swapped if low > high; at aperture 7 both are divided by 16 (cv::Canny scales that Sobel by
 * 1/16: see hc_derivatives_device); with l2gradient min(32767, t), then t * t for t > 0; then floored -- in this order, so
 * that L2 thresholds that are no multiples of 16 are exact at aperture 7 too (which integer context thresholds cannot
 * express).  The floored L1 thresholds are clamped to 32767; no L1 magnitude of any aperture on a u8 source reaches 32767
 * (at most 24480, at aperture 5), so the clamp changes no result.  Thresholds that are negative or not finite are HC_E_ARG.
 * Kernels: apertures 3 and 5 run what hc_run_device runs with HC_OPT_APERTURE 3 / 5 (same kernels, same bytes; hc_last_run_info
 * reports HC_FORM_FRONT8O / HC_FORM_FRONT_O / HC_FORM_O_APERTURE5).  Apertures 7 and -1 run k_front_o_ext's fused sources
 * (HC_FORM_O_APERTURE7 / HC_FORM_O_SCHARR): one kernel from the u8 frames to the bit planes, the derivatives (those of
 * hc_derivatives_device, bit for bit) never leave the registers -- no int16 planes to allocate, write and read back.
 * It is a run in every sense hc_run_device is one: pipeline slots and HC_OPT_PIPELINE, the stage timers (the front kernel's
 * time is divided over GRADIENT, NMS and THRESH, as for HC_FORM_O_APERTURE5), the hysteresis history and schedule,
 * hc_last_run_info, hc_set_stream, hc_set_tuning's rows per work item, HC_OPT_DEBUG_TAPS.
 * Views: exactly the rules of a HC_OPT_APERTURE 5 run of hc_run_device -- input rows without whole 4-pixel groups (pitch <
 * channels * round_up(width, 4)), pointers / pitches / frame strides that are no multiples of 4 and input views of 4 GiB
 * are staged; only [row, row + width) of every output row is written; the input is never written.
 * HC_E_ARG: a mode R context; an aperture outside {3, 5, 7, -1}; the thresholds above; otherwise whatever hc_run_device
 * gives for the same pointers, pitches and nframes. */
int hc_canny_device(hc_ctx *ctx, const void *d_in, size_t in_pitch, size_t in_frame_stride, void *d_out, size_t out_pitch,
                    size_t out_frame_stride, int nframes, double low, double high, int aperture, int l2gradient);

/* The derivatives cv::Canny(img, low, high, apertureSize, L2gradient) computes before its NMS, on their own (k_deriv16):
 * `d_in` holds nframes u8 frames of width * channels bytes per row (1 or 3 interleaved channels, as the context's);
 * `d_dx` / `d_dy` receive int16 planes with the same interleave (CV_16SC1 / CV_16SC3), both with `pitch` and `frame_stride`
 * in BYTES: the layout hc_run_gradients_device reads.  Chained with that entry, every apertureSize of cv::Canny runs on
 * the device: 3, 5, 7 and -1 (Scharr).  Contexts of either mode; width, height, channels and max_batch are the context's.
 * Semantics: those of canny.cpp's Sobel(src, dx, CV_16S, 1, 0, ksize, scale, 0, BORDER_REPLICATE) and Sobel(src, dy, CV_16S,
 * 0, 1, ...), restated (tests/deriv_ref.py) and, like all of Mode O, not pinned against a build of OpenCV.  Border indices
 * are clamped, the filter is a correlation; dx = derivative taps along x and smoothing taps along y, dy the other way round:
 *     ksize   smoothing taps         derivative taps        scale   range
 *       3     [1 2 1]                [-1 0 1]               1       +-1020
 *       5     [1 4 6 4 1]            [-1 -2 0 2 1]          1       +-12240
 *       7     [1 6 15 20 15 6 1]     [-1 -4 -5 0 5 4 1]     1/16    +-10200
 *      -1     [3 10 3]  (Scharr)     [-1 0 1]               1       +-4080
 * ksize 7: cv::Canny passes scale = 1/16; OpenCV filters in float (every intermediate is a multiple of 1/16 below 2^19, so
 * that path is exact) and converts with saturate_cast<short>(cvRound(v)).  The result is the exact integer sum S
 * (|S| <= 163200) divided by 16 and rounded HALF TO EVEN: (S + 7 + ((S >> 4) & 1)) >> 4 with an arithmetic shift.  The
 * unscaled 7x7 Sobel (cv::Sobel on its own) saturates int16 and is not offered.
 * Thresholds at 7: cv::Canny(img, low, high, 7) also divides low and high by 16 before it floors them.  The context
 * thresholds used with these derivatives are therefore in the SCALED units: a caller porting cv::Canny(img, low, high, 7)
 * sets floor(low / 16), floor(high / 16).  That mapping is exact for the L1 magnitude; with L2gradient (squared thresholds)
 * it is exact only for low / high that are multiples of 16.  This entry does not rescale thresholds; hc_canny_device, which
 * takes cv::Canny's own thresholds and aperture per call and fuses these derivatives into its front kernel, does.
 * Asynchronous on the context stream (hc_set_stream honoured), in order with everything else queued there: a following
 * hc_run_gradients_device on the same context needs no synchronisation in between, in plain and in pipelined mode.  It is not
 * a run: hc_last_run_info, the stage timers, the hysteresis schedule / history and the pipeline slots stay as they were, and
 * runs in flight are neither finished nor waited for.
 * Memory: no byte outside [row, row + channels * width) of an input row is read and none outside [row, row + 2 * channels *
 * width) of an output row is written -- never the rest of a pitch or the gap between frames -- so both sides may be ROIs
 * of larger images.  The input may have any alignment (rows that are not 4-byte aligned are read bytewise: slower, same
 * result); the outputs need even addresses, pitch and frame stride (8-byte aligned ones get the widest stores).
 * Rows are addressed with 32-bit offsets: a view with height * in_pitch >= 2^32 or height * pitch >= 2^32 is HC_E_ARG for
 * this entry (nothing is staged).  HC_E_ARG also for: a null pointer; odd d_dx / d_dy / pitch / frame_stride; in_pitch <
 * channels * width; pitch < 2 * channels * width; ksize not in {3, 5, 7, -1}; nframes outside 1..max_batch; nframes > 1
 * with a frame stride smaller than height * pitch on either side. */
int hc_derivatives_device(hc_ctx *ctx, const void *d_in, size_t in_pitch, size_t in_frame_stride, void *d_dx, void *d_dy,
                          size_t pitch, size_t frame_stride, int nframes, int ksize);

/* 256-bin histograms of u8 frames: d_hist[f][v] = number of samples of value v among the width * height * channels
 * samples of frame f (3-channel frames: all three channels pooled).  d_hist: uint32 [nframes][256], 4-byte aligned.
 * Contexts of either mode; width, height, channels and max_batch are the context's.  Asynchronous on the context stream
 * (hc_set_stream honoured), in order with everything else queued there; the entry zeroes d_hist on that stream first.  It is
 * not a run, exactly as hc_derivatives_device is none: hc_last_run_info, the stage timers, the hysteresis schedule /
 * history and the pipeline slots stay as they were, and runs in flight are neither finished nor waited for.
 * Views, as hc_derivatives_device: any alignment of base, pitch and frame stride (the dwords that lie whole inside a row
 * are read as dwords, the ragged head and tail bytewise); no byte outside [row, row + channels * width) of a row is read,
 * so `d_in` may be an ROI of a larger image.  Counts are integer sums: exact, whatever the work split (k_hist256).
 * HC_E_ARG: a null pointer; d_hist not 4-byte aligned; in_pitch < channels * width; nframes outside 1..max_batch; nframes
 * > 1 with a frame stride smaller than height * in_pitch; height * in_pitch >= 2^32. */
int hc_histogram_device(hc_ctx *ctx, const void *d_in, size_t in_pitch, size_t in_frame_stride, int nframes, void *d_hist);

/* Automatic thresholds per frame, on the device: the histogram of every frame (k_hist256, into a table the context owns:
 * allocated on first use, freed by hc_destroy), then one wave per frame turns it into the frame's (low, high) by `rule`
 * (k_auto_thr; the arithmetic is cudacam_amd/csrc/auto_thr.h, restated in tests/auto_thr_ref.py):
 *   HC_AUTO_MEDIAN, param = sigma in [0, 1] (the usual recipe: 0.33): with the N samples sorted, a = s[(N-1)/2],
 *     b = s[N/2], v = (a + b) / 2.0 (np.median, exact in double); low = (int)max(0.0, (1.0 - sigma) * v),
 *     high = (int)min(255.0, (1.0 + sigma) * v).
 *   HC_AUTO_OTSU, param = ratio in [0, 1] (the usual recipe: 0.5): high = t*, low = (int)(ratio * t*), where t* in 0..254
 *     is the smallest threshold whose between-class score ((double)d * (double)d) / ((double)w0 * (double)w1) is strictly the
 *     largest -- w0 = samples <= t, w1 = N - w0, d = S w0 - N s0 in int64 (S, s0: sums of the values of all samples / of those
 *     <= t) -- among the t with w0, w1 > 0; t* = 0 if there is none (a flat frame).  The textbook rule with an exact integer
 *     numerator, stated here; not pinned against OpenCV's getThreshVal_Otsu_8u, which accumulates in floating point and
 *     may differ at near-ties.
 * d_thr: int32 [nframes][2], 4-byte aligned, as hc_frame_thresholds_device reads it, in the units of hc_set_thresholds.  With
 * derivatives of aperture 7 or Scharr (hc_derivatives_device chained with hc_run_gradients_device) the pairs mean what that
 * entry says about units; nothing is rescaled here.  Asynchronous on the context stream, not a run (as hc_histogram_device):
 * chained with hc_frame_thresholds_device and a run on the same context, no synchronisation is needed in between.
 * Successive calls on one context share that table and are ordered by the stream they are queued on; a change of the stream
 * between two calls (hc_set_stream, hc_use_own_stream) keeps that order, since the switch queues the incoming stream behind
 * the outgoing one.  Work the caller queues itself on a third stream it orders itself, as for any other memory that two
 * streams touch; hc_histogram_device, which writes caller memory only, has no such state.
 * HC_E_ARG: an unknown rule; param outside [0, 1] or not finite; width * height * channels > 2^27 (up to there the integer
 * sums above are exact); d_thr null or not 4-byte aligned; otherwise what hc_histogram_device refuses. */
enum { HC_AUTO_MEDIAN = 0, HC_AUTO_OTSU = 1 };
int hc_auto_thresholds_device(hc_ctx *ctx, const void *d_in, size_t in_pitch, size_t in_frame_stride, int nframes,
                              int rule, double param, void *d_thr /* int32 [nframes][2], as hc_frame_thresholds_device reads */);

/* The edge pixels of u8 maps as point lists and counts, on the device: cv::findNonZero / cv::countNonZero per frame
 * (k_edge_count, k_edge_scan, k_edge_emit: cudacam_amd/csrc/edge_points.hip).  Semantics stated here and restated in
 * tests/edge_points_ref.py (numpy), not pinned against a build of OpenCV.
 * `d_map` holds nframes u8 images of the context's width x height with ONE channel, whatever `channels` the context has (an
 * edge map is single-channel; after an HC_OPT_PER_CHANNEL run the caller passes its 3 maps per input frame).  A pixel belongs to
 * the list iff its byte is non-zero: the 255 of a final map, and the 128 and 255 of an HC_STAGE_THRESH map alike.
 *   d_counts[f]  uint32: the number of non-zero pixels of frame f -- always the full number, also above `capacity`.
 *   d_points     int32 [nframes][capacity][2]: the slot of frame f, at byte f * capacity * 8, receives the first
 *                min(d_counts[f], capacity) points of the frame in raster order (rows top to bottom, columns left to right
 *                inside a row), each as (int32 x, int32 y) -- the memory of a cv::Mat(count, 1, CV_32SC2) / a
 *                std::vector<cv::Point> as cv::findNonZero fills it.
 * Nothing else is written: the bytes of a slot behind its written points, the other slots and the map stay untouched.
 * capacity == 0 (d_points null or not) gives the counts only: cv::countNonZero per frame.  The order is part of the contract:
 * the result is a function of the map alone, whatever the work split.
 * Views, as hc_histogram_device: any alignment of base, pitch and frame stride; no byte outside [row, row + width) of a row is
 * read, so `d_map` may be an ROI of a larger image.  d_counts is 4-byte aligned, d_points 8-byte aligned.
 * Asynchronous on the context stream (hc_set_stream honoured), in order with everything else queued there.  It is not a run,
 * exactly as hc_histogram_device is none: hc_last_run_info, the stage timers, the hysteresis schedule / history and the pipeline
 * slots stay as they were.  One addition, because a run's output is this entry's natural input: with HC_OPT_PIPELINE, a run
 * still in flight whose output overlaps the bytes of `d_map` is completed first (its hysteresis runs on another stream and may
 * be continued from the host), as a later run that writes there would complete it; runs whose outputs do not overlap are
 * neither finished nor waited for.  In plain mode the order of the context stream suffices (as for any reader of a plain run's
 * output on that stream: a run that had to be continued from the host, hc_last_hysteresis_info, is complete after hc_sync).
 * Scratch: one table of per-work-item counts the context owns (allocated on first use, freed by hc_destroy).  Successive calls
 * on one context share it and are ordered by the stream they are queued on, across a change of the stream (hc_set_stream,
 * hc_use_own_stream) too, as for hc_auto_thresholds_device.
 * HC_E_ARG: ctx, d_map or d_counts null; d_points null with capacity > 0; d_counts not 4-byte / d_points not 8-byte aligned;
 * pitch < width; nframes outside 1..(output frames of a max_batch run: max_batch, 3 * max_batch with HC_OPT_PER_CHANNEL);
 * nframes > 1 with a frame stride smaller than height * pitch; height * pitch >= 2^32; capacity * 8 * nframes overflowing
 * size_t. */
int hc_edge_points_device(hc_ctx *ctx, const void *d_map, size_t pitch, size_t frame_stride, int nframes,
                          void *d_counts /* uint32 [nframes] */,
                          void *d_points /* int32 [nframes][capacity][2] = (x, y); may be NULL when capacity == 0 */,
                          size_t capacity);

/* cv::GaussianBlur(src, dst, Size(ksize, ksize), sigma) for CV_8U frames on the device -- the step almost every cv::Canny
 * caller runs first, cv::Canny having no smoothing of its own (k_gauss8: cudacam_amd/csrc/blur.hip).  The semantics are stated
 * here and restated in tests/gauss_blur_ref.py (numpy); like the rest of Mode O they are not pinned against a build of OpenCV.
 * Taps: K = ksize is 3, 5 or 7; the same K taps serve x and y.  `taps` points to K uint16 values t[0 .. K-1] in HOST memory
 * (read before the call returns), Q8 fixed point: 256 = 1.0, each tap <= 256, their sum exactly 256; symmetry is not required.
 * Filter: a correlation -- tap i multiplies the pixel i - K/2 columns (rows) from the output pixel; the channels of 3-channel
 * frames filter independently and stay interleaved.  Per pixel and channel:
 *     h   = sum_i t[i] * src      along the row      (exact in 16 bits unsigned: at most 255 * 256 = 65280)
 *     v   = sum_j t[j] * h        along the column   (exact in 32 bits: below 2^24)
 *     out = (v + 32768) >> 16
 * which is cv::GaussianBlur's fixed-point path for CV_8U: 8.8 coefficients, a 16.16 accumulator, rounding by adding one half.
 * Constant frames come back unchanged.
 * Border: HC_BORDER_REFLECT_101 (cv::GaussianBlur's default: gfedcb|abcdefgh|gfedcba) or HC_BORDER_REPLICATE (aaaaaa|abcdefgh|
 * hhhhhhh), as cv::borderInterpolate defines them: an index outside the axis is clamped, or reflected about the edge pixels
 * without repeating them until it lies inside; an axis of length 1 maps to index 0.  That is np.pad(mode="reflect") /
 * np.pad(mode="edge"), axes shorter than the radius included.
 * Contexts of either mode; width, height, channels and max_batch are the context's.  Both views are u8 rows of channels * width
 * bytes with any alignment of base, pitch and frame stride (4-byte aligned ones get dword loads / stores); no byte outside
 * [row, row + channels * width) of a row is read or written on either side, so both may be ROIs of larger images.  Rows are
 * addressed with 32-bit offsets: height * pitch >= 2^32 on either side is HC_E_ARG.  The byte ranges of the two views must not
 * overlap: in-place operation is refused, not staged (cv::GaussianBlur clones its source in that case; this entry owns no
 * scratch) -- views that merely touch, one ending where the other begins, are fine.
 * Asynchronous on the context stream (hc_set_stream honoured), in order with everything else queued there: a following
 * hc_canny_device / hc_run_device that reads d_out needs no synchronisation in between.  It is not a run, exactly as
 * hc_derivatives_device is none: hc_last_run_info, the stage timers, the hysteresis schedule / history and the pipeline slots
 * stay as they were.  One addition, as for hc_edge_points_device: with HC_OPT_PIPELINE, a run still in flight whose output
 * overlaps either view is completed first.
 * HC_E_ARG: a null pointer; ksize not in {3, 5, 7}; a border outside the enum; a tap above 256 or a tap sum other than 256; a
 * pitch < channels * width; nframes outside 1..max_batch; nframes > 1 with a frame stride smaller than height * pitch; height *
 * pitch >= 2^32; overlapping views. */
enum { HC_BORDER_REFLECT_101 = 0, HC_BORDER_REPLICATE = 1 };
int hc_gaussian_blur_device(hc_ctx *ctx, const void *d_in, size_t in_pitch, size_t in_frame_stride, void *d_out, size_t out_pitch,
                            size_t out_frame_stride, int nframes, int ksize, const uint16_t *taps /* host, ksize values */, int border);

/* The Q8 taps of a Gaussian for the entry above, on the host (no context, no GPU): cv::getGaussianKernel followed by the 8.8
 * conversion of cv::GaussianBlur's fixed-point path, restated; not pinned against a build of OpenCV.  With K = ksize (3, 5, 7):
 *   sigma <= 0: OpenCV's small fixed kernels times 256: [64 128 64], [16 64 96 64 16], [8 28 56 72 56 28 8].
 *   sigma > 0:  g[i] = exp(-(i - K/2)^2 / (2 sigma^2)) for i = 0 .. K-1 (the centre is 1; where 2 sigma^2 underflows to 0 the
 *     others are 0), divided by their sum (added in that order), all in double.  From the outside inwards, i = 0 .. K/2 - 1, with err = 0 at the start: x = 256 g[i] + err, v = nearbyint(x)
 *     (round half to even), err = x - v, t[i] = t[K-1-i] = v.  The centre tap is 256 minus the sum of the others.
 * The result is symmetric and sums to 256.  HC_E_ARG: taps null; ksize not in {3, 5, 7}; a sigma that is not finite, or one
 * whose taps would leave 0 .. 256. */
int hc_gaussian_taps_q8(int ksize, double sigma, uint16_t *taps);

/* cv::HoughLines(edges, lines, rho, theta, threshold, 0, 0, min_theta, max_theta) -- the standard transform, srn = stn = 0 -- on
 * the device, fed by the point lists of hc_edge_points_device (k_hough_vote, k_hough_peaks, k_hough_scan, k_hough_rank:
 * cudacam_amd/csrc/hough.hip).  One call returns per frame the number of lines and the strongest of them as (rho, theta, votes)
 * in cv::HoughLines' order.  The semantics are stated here and restated in tests/hough_ref.py (numpy); like the rest of Mode O
 * they are not pinned against a build of OpenCV.  Out of scope: cv::HoughLines' multi-scale form (srn / stn other than 0),
 * cv::HoughLinesP's progressive probabilistic transform (segments: hc_hough_segments_device below; circles: hc_hough_circles_device).
 * With W, H the context's frame size and rho, theta, min_theta, max_theta doubles:
 * Geometry.  numangle = floor((max_theta - min_theta) / theta) + 1; if numangle > 1 and |pi - (numangle - 1) * theta| < theta / 2
 *   it is one less.  numrho = rint((2 * (W + H) + 1) / rho), half to even.  (1920 x 1080, rho 1, theta pi / 180, [0, pi]: 180, 6001.)
 * Tables.  irho = 1.0f / (float)rho; ang = (float)min_theta; for n = 0 .. numangle - 1: tab_cos[n] = (float)(cos((double)ang) *
 *   (double)irho), tab_sin[n] likewise with sin, tab_theta[n] = ang, then ang += (float)theta in float.  cos / sin are libm's, on
 *   the host (hc_hough_tables below is the function the device entry itself uses).
 * Votes.  The accumulator is int32 [numangle + 2][numrho + 2], zero to begin with.  A point is (int32 x, int32 y).  For each n:
 *   r = rint((float)x * tab_cos[n] + (float)y * tab_sin[n]) -- two float32 products, each rounded, and one float32 sum, no fused
 *   multiply-add, rint half to even -- then r += (numrho - 1) / 2 (integer division) and accum[n + 1][r + 1] += 1.  A vote whose r
 *   falls outside -1 .. numrho is dropped: no coordinate, whatever the caller passes, writes outside the accumulator.  For points
 *   inside the frame no vote is dropped.
 * Peaks.  Cell (n, r), 0 <= n < numangle, 0 <= r < numrho, with value a = accum[n + 1][r + 1] is a line iff a > threshold, a >
 *   accum[n + 1][r] (left), a >= accum[n + 1][r + 2] (right), a > accum[n][r + 1] (up) and a >= accum[n + 2][r + 1] (down); the
 *   padding cells take part as neighbours.
 * Order.  Votes descending, ties by ascending accumulator index (n + 1) * (numrho + 2) + r + 1.  The keys are unique: the order
 *   is total and a function of the input alone.
 * Output.  d_line_counts[f] (uint32) is always the full number of peaks of frame f.  d_lines is float32 [nframes][line_capacity]
 *   [3]: the slot of frame f receives its first min(count, line_capacity) lines in that order, each as ((r - (numrho - 1) * 0.5f) *
 *   (float)rho, tab_theta[n], (float)votes) -- the memory of the CV_32FC3 matrix cv::HoughLines fills.  Nothing else is written.
 *   line_capacity == 0 (d_lines null or not) gives the counts only.
 * Input.  d_points (int32 [nframes][point_capacity][2], 8-byte aligned) and d_point_counts (uint32 [nframes]) are exactly what
 *   hc_edge_points_device wrote: frame f votes with its first min(d_point_counts[f], point_capacity) points.  A list that was cut
 *   by its capacity votes with what it holds -- the lines are then those of the cut list, not of the map.  Neither is written.
 * Asynchronous on the context stream (hc_set_stream honoured), in order with everything else queued there: chained behind
 * hc_canny_device and hc_edge_points_device it needs no synchronisation.  Contexts of either mode.  It is not a run, exactly as
 * hc_edge_points_device is none (hc_last_run_info, the stage timers, the hysteresis schedule / history and the pipeline slots
 * stay as they were), and since no run writes a point list, no run in flight is completed first.
 * Scratch, owned by the context, allocated on first use and freed by hc_destroy: the tables on the device (made again, after a
 * synchronisation of the context stream, only when rho, theta, min_theta or max_theta differ from the call before), and per
 * frame of a pass the accumulator, the compacted peak list (at most ceil(numrho / 2) peaks per angle row, two horizontal
 * neighbours never being both peaks) and a count per angle row.  The scratch is bounded at 256 MiB: a batch is cut into passes
 * of as many frames as fit, 65535 at most (a 1080p accumulator is 4.4 MB) and is allocated again, after a synchronisation, when a call needs more
 * than the calls before.  Successive calls on one context share scratch and tables and are ordered by the stream they are
 * queued on, across a change of the stream (hc_set_stream, hc_use_own_stream) too, as for hc_auto_thresholds_device.
 * Cost.  Votes: points x numangle LDS atomics per frame; an accumulator row lives in one workgroup's LDS.  The ranking compares
 * every peak of a frame with every other: quadratic in the peaks -- a few hundred at any threshold in use, a few 10^5 only at threshold 0
 * on large noisy frames (measured on an MI355X: 0.4 ms per frame at 56 k peaks, profiles/hough/README.md; extrapolated by the
 * square, not measured: about 10 ms at 3 x 10^5).  It is not launched when line_capacity == 0.
 * HC_E_ARG: ctx, d_points, d_point_counts or d_line_counts null; d_lines null with line_capacity > 0; d_points not 8-byte,
 * another pointer not 4-byte aligned; nframes outside 1..(max_batch, 3 * max_batch with HC_OPT_PER_CHANNEL); rho or theta <= 0
 * or not finite; max_theta < min_theta or either not finite; threshold < 0; an accumulator row of (numrho + 2) * 4 bytes that
 * does not fit one workgroup's LDS (160 KiB); (numangle + 2) * (numrho + 2) >= 2^31; one frame's scratch above the bound;
 * point_capacity * 8 * nframes or line_capacity * 12 * nframes overflowing size_t. */
int hc_hough_lines_device(hc_ctx *ctx, const void *d_points /* int32 [nframes][point_capacity][2] */,
                          const void *d_point_counts /* uint32 [nframes] */, size_t point_capacity, int nframes, double rho, double theta,
                          int threshold, double min_theta, double max_theta, void *d_line_counts /* uint32 [nframes] */,
                          void *d_lines /* float32 [nframes][line_capacity][3]; may be NULL when line_capacity == 0 */, size_t line_capacity);

/* Geometry and tables of the entry above, on the host (no context, no GPU), by the rule stated there.  *numangle and *numrho are
 * always written on success.  The tables are given together or not at all (all three null: the geometry only); each receives
 * numangle floats, and table_capacity, the floats each can hold, must be at least numangle.  HC_E_ARG, with nothing written:
 * numangle or numrho null; only some tables given; width or height < 1; the rho / theta / min_theta / max_theta and accumulator
 * refusals of hc_hough_lines_device; table_capacity < numangle. */
int hc_hough_tables(int width, int height, double rho, double theta, double min_theta, double max_theta, int *numangle, int *numrho,
                    float *tab_cos, float *tab_sin, float *tab_theta, size_t table_capacity);

/* Line segments from the lines of hc_hough_lines_device: every line is walked across the edge map and the walk is cut into
 * segments by a largest gap and a smallest length (k_seg_count, k_seg_scan, k_seg_emit: cudacam_amd/csrc/hough_segments.hip).
 * This is the form of cv::cuda::HoughSegmentDetector, not cv::HoughLinesP: that one is a sequential transform driven by a random
 * number generator, whose result is no function of its input alone.  The semantics are stated here and restated in
 * tests/hough_segments_ref.py (numpy); like the rest of Mode O they are not pinned against a build of OpenCV.
 * With W, H the context's frame size:
 * Input.  d_map is what hc_edge_points_device reads: one-channel u8 maps of W x H in a pitched view; a pixel is an edge iff its
 *   byte is non-zero.  d_lines (float32 [nframes][line_capacity][3]) and d_line_counts (uint32 [nframes]) are exactly what
 *   hc_hough_lines_device wrote: frame f walks its first min(d_line_counts[f], line_capacity) lines.  rho, theta, min_theta and
 *   max_theta are those of the call that made the lines: they give numangle and tab_theta by the rule of hc_hough_tables.
 *   Neither the map nor the lines are written.
 * Angle of a line.  Its index is the smallest n with tab_theta[n] equal to the line's second float bit for bit (the lines carry
 *   copies of the table's entries).  A line whose theta equals no entry -- a NaN included -- yields no segments.  The device
 *   computes no trigonometry.
 * Walk tables, on the host (hc_hough_walk_tables below is the function the device entry itself uses).  For angle n: a =
 *   (double)tab_theta[n], c = cos(a), s = sin(a) (libm, double).  If fabs(s) >= fabs(c): major[n] = 0 (x-major: one sample per
 *   column), slope[n] = (float)(-c / s), scale[n] = (float)(1.0 / s).  Otherwise major[n] = 1 (y-major: one sample per row),
 *   slope[n] = (float)(-s / c), scale[n] = (float)(1.0 / c).  |slope| <= 1 either way.
 * Samples.  L = W, M = H when x-major; L = H, M = W when y-major.  For step t = 0 .. L - 1: m = rint((float)t * slope[n] + line_rho
 *   * scale[n]) -- two float32 products, each rounded, and one float32 sum, no fused multiply-add, rint half to even --, line_rho
 *   being the line's first float, in pixels.  The sample is pixel (t, m) when x-major and (m, t) when y-major.  The range test
 *   0 <= m <= M - 1 is made on the float, as a comparison of real numbers, before any conversion: a rho of any size, infinities
 *   and NaNs address nothing.  A sample outside the frame is not an edge.
 * Segments.  Let t_1 < t_2 < ... be the steps whose sample is an edge.  A new group starts at t_1 and at every t_(k+1) with
 *   t_(k+1) - t_k - 1 > max_gap.  A group is a candidate segment from its first sample (x0, y0) to its last (x1, y1), and is kept
 *   iff (x1 - x0)^2 + (y1 - y0)^2 >= min_length^2 in 64-bit integers: a group of one sample only when min_length == 0.
 * Order.  By line, in the order of d_lines; within a line by ascending t.  A function of the input alone.
 * Output.  d_seg_counts[f] (uint32) is always the full number of kept segments of frame f.  d_segs is int32 [nframes]
 *   [seg_capacity][4]: the slot of frame f, at byte f * seg_capacity * 16, receives its first min(count, seg_capacity) segments as
 *   (x0, y0, x1, y1) -- the memory of the std::vector<cv::Vec4i> cv::HoughLinesP fills.  Nothing else is written.  seg_capacity
 *   == 0 (d_segs null or not) gives the counts only.
 * Asynchronous on the context stream (hc_set_stream honoured), in order with everything else queued there: chained behind
 * hc_canny_device, hc_edge_points_device and hc_hough_lines_device it needs no synchronisation.  Contexts of either mode.  It is
 * not a run, exactly as hc_edge_points_device is none, and like it completes first a pipelined run still in flight whose output
 * overlaps d_map.  The view follows hc_edge_points_device: any alignment of base, pitch and frame stride, no byte outside [row,
 * row + width) of a row is read, rows are addressed with 32-bit offsets.
 * Scratch, owned by the context, allocated on first use and freed by hc_destroy: a count per line slot (uint32 [nframes]
 * [line_capacity], allocated again after a synchronisation when a call needs more) and the tables on the device (made again,
 * after a synchronisation of the context stream, only when rho, theta, min_theta or max_theta differ from the call before).
 * Successive calls on one context share both and are ordered by the stream they are queued on, as for hc_hough_lines_device.
 * Cost.  A wave per line slot, 64 steps per trip; a y-major walk reads one cache line per step.
 * HC_E_ARG: ctx, d_map, d_lines, d_line_counts or d_seg_counts null; d_segs null with seg_capacity > 0; d_lines, d_line_counts
 * or d_seg_counts not 4-byte, d_segs not 16-byte aligned; min_length < 0 or max_gap < 0; the view and nframes refusals of
 * hc_edge_points_device; the rho, theta, min_theta, max_theta and accumulator refusals of hc_hough_lines_device; line_capacity
 * == 0; line_capacity * 12 * nframes, line_capacity * 4 * nframes or seg_capacity * 16 * nframes overflowing size_t; nframes *
 * line_capacity above 2^31 - 16 line slots; line_capacity * ceil(max(W, H) / 2) >= 2^32 (a frame's count would not fit). */
int hc_hough_segments_device(hc_ctx *ctx, const void *d_map, size_t pitch, size_t frame_stride,
                             const void *d_lines /* float32 [nframes][line_capacity][3] */, const void *d_line_counts /* uint32 [nframes] */,
                             size_t line_capacity, int nframes, double rho, double theta, double min_theta, double max_theta,
                             int min_length, int max_gap, void *d_seg_counts /* uint32 [nframes] */,
                             void *d_segs /* int32 [nframes][seg_capacity][4] = (x0, y0, x1, y1); may be NULL when seg_capacity == 0 */, size_t seg_capacity);

/* The walk tables of the entry above, on the host (no context, no GPU), by the rule stated there.  *numangle is always written
 * on success.  The tables are given together or not at all (all three null: numangle only); each receives numangle values, and
 * table_capacity, the values each can hold, must be at least numangle.  HC_E_ARG, with nothing written: numangle null; only some
 * tables given; width or height < 1; the rho / theta / min_theta / max_theta and accumulator refusals of hc_hough_lines_device;
 * table_capacity < numangle. */
int hc_hough_walk_tables(int width, int height, double rho, double theta, double min_theta, double max_theta,
                         int *numangle, int32_t *major, float *slope, float *scale, size_t table_capacity);   /* host, no context, no GPU */

/* Circles from the edge point lists of hc_edge_points_device and the gradient planes cv::Canny itself uses: centres voted along
 * the gradient, sifted by a smallest distance, and a radius histogram per kept centre (k_circle_vote, k_hough_peaks, k_hough_scan,
 * k_circle_rank, k_circle_sift, k_circle_radii, k_circle_scan: cudacam_amd/csrc/hough_circles.hip).  This is the form of
 * cv::cuda::HoughCirclesDetector, not cv::HoughCircles, which is no fixed function of its input across OpenCV versions.  The
 * semantics are stated here and restated in tests/hough_circles_ref.py (numpy); like the rest of Mode O they are not pinned
 * against a build of OpenCV.  Out of scope: HOUGH_GRADIENT_ALT, param1 (the caller runs cv::Canny with its own thresholds),
 * 3-channel gradient planes, sub-cell refinement of the centres.  With W, H the context's frame size:
 * Geometry (hc_hough_circle_geometry below is the function the device entry itself uses).  idp = 1.0f / (float)dp.  AW =
 *   ceil((double)((float)W * idp)), AH likewise from H.  The accumulator is int32 [AH + 2][AW + 2], zero to begin with.  min_d2 is
 *   the smallest int64 q with (double)q >= md * md, where md = min_dist / dp in double (min_dist 0 gives 0); a bound of 2^62 and
 *   more is 2^62: no two cells lie that far apart.
 * Input.  d_points (int32 [nframes][point_capacity][2] = (x, y), 8-byte aligned) and d_point_counts (uint32 [nframes]) are exactly
 *   what hc_edge_points_device wrote: frame f uses its first min(d_point_counts[f], point_capacity) points.  d_dx / d_dy are
 *   one-channel int16 planes of W x H with a common pitch and frame stride in bytes: what hc_derivatives_device writes on a
 *   1-channel context.  A point outside 0 <= x < W, 0 <= y < H takes part in nothing: it reads no gradient, casts no vote and
 *   counts in no histogram.  No coordinate a caller can pass makes the entry read or write outside its views.  Nothing of the input
 *   is written.
 * Centre votes.  For each point with the gradient (vx, vy) read at (x, y), skipped when both are 0: m = (uint32)(vx * vx + vy * vy)
 *   (exact; at most 2^31), mag = sqrtf((float)m), correctly rounded; x0 = rint(((float)x * idp) * 1024.0f), sx = rint((((float)vx *
 *   idp) * 1024.0f) / mag), and likewise y0, sy.  Every product, the quotient and the square root are single float32 operations,
 *   each rounded to nearest, no fused multiply-add; rint rounds half to even.  Both directions d = +1, -1: x1 = x0 + d * min_radius
 *   * sx, y1 likewise; then for r = min_radius .. max_radius: x2 = x1 >> 10, y2 = y1 >> 10 (arithmetic shifts); the direction ends
 *   at the first (x2, y2) outside 0 .. AW - 1 x 0 .. AH - 1; otherwise accum[y2 + 1][x2 + 1] += 1, then x1 += d * sx, y1 += d * sy.
 *   All of this is int32; the refusals below keep it from overflowing (|sx|, |sy| <= 1024).
 * Centres.  Cell (cx, cy), 0 <= cx < AW, 0 <= cy < AH, with value a = accum[cy + 1][cx + 1] is a centre iff a > votes_threshold, a
 *   > accum[cy][cx + 1] (up), a >= accum[cy + 2][cx + 1] (down), a > accum[cy + 1][cx] (left) and a >= accum[cy + 1][cx + 2]
 *   (right); the padding cells take part as neighbours.  The rule of hc_hough_lines_device, with rows = AH and columns = AW.
 * Centre order.  Votes descending, ties by ascending index (cy + 1) * (AW + 2) + cx + 1.  Only the first centre_capacity centres in
 *   that order go on.
 * Smallest distance.  Those centres are gone through in that order: one is kept iff every centre kept before it has (cx - cx')^2
 *   + (cy - cy')^2 >= min_d2, in int64.
 * Radii.  For each kept centre, in that order: fx = ((float)cx + 0.5f) * (float)dp, fy likewise.  hist[0 .. max_radius -
 *   min_radius + 2] is zero to begin with.  For every point of the frame inside the frame: ddx = fx - (float)x, ddy = fy - (float)y,
 *   rad = sqrtf(ddx * ddx + ddy * ddy) -- two rounded products, one rounded sum, a correctly rounded root, no fused multiply-add
 *   --; if rad >= (float)min_radius && rad <= (float)max_radius then hist[(int)rint(rad - (float)min_radius) + 1] += 1.  Radius
 *   index i = 0 .. max_radius - min_radius is a circle iff h = hist[i + 1] has h >= votes_threshold, h > hist[i] and h >= hist[i + 2].
 * Output.  Circles are ordered by centre, in the order above, and within a centre by ascending radius: a function of the input
 *   alone.  d_circle_counts[f] (uint32) is always the full number of circles of frame f.  d_circles is float32 [nframes]
 *   [circle_capacity][4]: the slot of frame f, at byte f * circle_capacity * 16, receives its first min(count, circle_capacity)
 *   circles as (fx, fy, (float)(i + min_radius), (float)h).  Nothing else is written.  circle_capacity == 0 (d_circles null or
 *   not) gives the counts only.
 * Asynchronous on the context stream (hc_set_stream honoured), in order with everything else queued there: chained behind
 * hc_derivatives_device, hc_canny_device and hc_edge_points_device it needs no synchronisation.  Contexts of either mode.  It is
 * not a run, exactly as hc_hough_lines_device is none, and since no run writes a point list or a gradient plane, no run in flight
 * is completed first.
 * Scratch, owned by the context, allocated on first use and freed by hc_destroy, per frame of a pass: the accumulator (zeroed on
 * the context stream before the votes), the compacted peak list (at most AH * ceil(AW / 2) peaks), a count per accumulator row,
 * the ranked and the kept centres (centre_capacity of 16 bytes each), a count per centre.  It is bounded by the bound of
 * hc_hough_lines_device (256 MiB): a batch is cut into passes of as many frames as fit, 65535 at most, and the scratch is
 * allocated again, after a synchronisation, when a call needs more than the calls before.  Successive calls on one context share
 * it and are ordered by the stream they are queued on, across a change of the stream (hc_set_stream, hc_use_own_stream) too,
 * as for hc_hough_lines_device.
 * Cost.  Votes: up to 2 * (max_radius - min_radius + 1) global atomic adds per point.  The ranking is quadratic in the peaks of a
 * frame, as for hc_hough_lines_device.  The sift is sequential: one wave per frame.  Every kept centre reads the frame's point
 * list once per radii launch (twice when circles are written).  Measurements: profiles/hough_circles/README.md.
 * HC_E_ARG: ctx, d_points, d_point_counts, d_dx, d_dy or d_circle_counts null; d_circles null with circle_capacity > 0; d_points
 * not 8-byte, d_point_counts or d_circle_counts not 4-byte, d_circles not 16-byte aligned; d_dx, d_dy, pitch or frame_stride odd;
 * pitch < 2 * W; H * pitch >= 2^32; nframes > 1 with frame_stride < H * pitch; a view that wraps the address space; nframes outside
 * 1..(max_batch, 3 * max_batch with HC_OPT_PER_CHANNEL); dp < 1 or not finite, or so large that AW or AH is 0; min_dist < 0 or not
 * finite; votes_threshold < 0; min_radius < 1; max_radius < min_radius; max_radius - min_radius + 3 > 4096 histogram words; W +
 * max_radius >= 2^20 or H + max_radius >= 2^20; centre_capacity outside 1..4096; (AH + 2) * (AW + 2) >= 2^31; one frame's scratch
 * above the bound; point_capacity * 8 * nframes or circle_capacity * 16 * nframes overflowing size_t. */
int hc_hough_circles_device(hc_ctx *ctx, const void *d_points /* int32 [nframes][point_capacity][2] */,
                            const void *d_point_counts /* uint32 [nframes] */, size_t point_capacity, const void *d_dx, const void *d_dy,
                            size_t pitch, size_t frame_stride /* int16, ONE channel, W x H, bytes */, int nframes, double dp, double min_dist,
                            int votes_threshold, int min_radius, int max_radius, size_t centre_capacity, void *d_circle_counts /* uint32 [nframes] */,
                            void *d_circles /* float32 [nframes][circle_capacity][4] = (x, y, radius, votes); may be NULL when circle_capacity == 0 */,
                            size_t circle_capacity);

/* The geometry of the entry above, on the host (no context, no GPU), by the rule stated there: all three numbers are written on
 * success.  HC_E_ARG, with nothing written: a null pointer; width or height < 1; the dp, min_dist, min_radius, max_radius, 2^20
 * and accumulator refusals of hc_hough_circles_device. */
int hc_hough_circle_geometry(int width, int height, double dp, double min_dist, int min_radius, int max_radius,
                             int *acc_width, int *acc_height, long long *min_d2);   /* host, no context, no GPU */

/* The connected components of u8 maps on the device: a number per pixel, the number of components and, per component, bounding
 * box, area and centroid -- cv::connectedComponents / cv::connectedComponentsWithStats per frame, the form OpenCV's GPU module
 * offers as cv::cuda::connectedComponents (k_ccl_local, k_ccl_merge, k_ccl_flatten, k_ccl_scan, k_ccl_roots, k_ccl_number,
 * k_ccl_rows, k_ccl_stats, k_ccl_finish: cudacam_amd/csrc/ccl.hip).  The semantics are stated here and restated in
 * tests/ccl_ref.py (numpy and a flood fill); like the rest of Mode O they are not pinned against a build of OpenCV.  With W, H the
 * context's frame size:
 * Input.  d_map is what hc_edge_points_device reads: one-channel u8 maps of W x H in a pitched view, whatever `channels` the
 *   context has; any alignment of base, pitch and frame stride; no byte outside [row, row + W) of a row is read.  A pixel is
 *   foreground iff its byte is non-zero: the 255 of a final map, the 128 / 255 of an HC_STAGE_THRESH map alike.  The map is never
 *   written.
 * Connectivity.  8: neighbours share an edge or a corner (OpenCV's default); 4: an edge only.  A component is a maximal set of
 *   foreground pixels connected through such neighbours inside the frame.  Frames are independent.
 * Numbering.  The first pixel of a component is its pixel with the smallest y * W + x; components are numbered 1, 2, ... in
 *   ascending order of their first pixels; background is 0.  This is the order a raster scan meets them in, and the order
 *   scipy.ndimage.label gives.  cv::connectedComponents promises no order: a caller who compares with it compares partitions.
 * Labels.  d_labels receives int32 [H][W] per frame, label_pitch and label_frame_stride in bytes -- the memory of a CV_32S
 *   cv::Mat.  Exactly the bytes [row, row + 4 * W) of every row are written, so it may be an ROI of a larger plane; base, pitch
 *   and frame stride are multiples of 4 (nothing is staged).  Required; CV_16U labels are not offered.  Every pixel gets its final
 *   number, also the pixels of components numbered `capacity` and above.  While the call runs the plane holds intermediate links.
 * Counts.  d_counts[f] = N = components + 1, the value cv::connectedComponents returns (background included) -- always the full
 *   number, also above `capacity`.
 * Stats and centroids.  The slots of frame f start at bytes f * capacity * 20 and f * capacity * 16 and receive the rows
 *   0 .. min(N, capacity) - 1; row 0 is the background, row k component k -- the memory of the CV_32S N x 5 and CV_64F N x 2
 *   matrices of cv::connectedComponentsWithStats.  HC_CC_STAT_LEFT / TOP: the smallest x / y; WIDTH / HEIGHT: largest minus
 *   smallest plus 1; AREA: the pixel count.  Centroid = ((double)sx / (double)area, (double)sy / (double)area) with sx, sy the
 *   exact int64 sums of the pixels' x and y: one correctly rounded float64 division each.  A background without a pixel (a full
 *   frame) gets five zeros and the centroid (0.0, 0.0); OpenCV leaves its initial values (INT_MAX / INT_MIN boxes, a 0 / 0
 *   centroid) there.  Nothing else is written: not the rows behind a slot's written rows, not other slots.  The written rows hold
 *   intermediate sums while the call runs.  capacity == 0 (pointers null or not) gives labels and counts only:
 *   cv::connectedComponents.  d_stats is 4-byte, d_centroids 8-byte aligned; both are required when capacity > 0.
 * Asynchronous on the context stream (hc_set_stream honoured).  Chained behind hc_canny_device it needs no synchronisation.
 * Contexts of either mode.  It is not a run, exactly as hc_edge_points_device is none (hc_last_run_info, the stage timers, the
 * hysteresis schedule / history and the pipeline slots stay as they were), and as hc_gaussian_blur_device does for both of its
 * views it completes first a pipelined run still in flight whose output overlaps d_map or the label view.
 * The result is a function of the map alone although the kernels merge with global atomics: the fixed point of a min-label
 * union-find is unique (every component ends rooted at its first pixel), the numbering is a total order, and integer sums, minima
 * and maxima do not depend on arrival order.
 * Scratch: one table of per-row-chunk counts the context owns (allocated on first use, grown when a call needs more, freed by
 * hc_destroy; 4 bytes per 8 to 64 rows of a frame), under the bound of hc_hough_lines_device's scratch (256 MiB; a batch whose
 * tables exceed it runs in passes of as many frames as fit).  The only per-pixel storage is the label plane.  Successive calls
 * share the table and are ordered by the stream they are queued on, as for hc_edge_points_device.
 * HC_E_ARG: ctx, d_map, d_labels or d_counts null; d_stats or d_centroids null with capacity > 0; connectivity not 4 or 8;
 * d_counts or d_stats not 4-byte, d_centroids not 8-byte aligned; d_labels, label_pitch or label_frame_stride no multiple of 4;
 * pitch < W; label_pitch < 4 * W; H * pitch >= 2^32 or H * label_pitch >= 2^32; nframes outside 1..(max_batch, 3 * max_batch with
 * HC_OPT_PER_CHANNEL); nframes > 1 with a frame stride below H * pitch on either side; a view that wraps the address space;
 * W * H >= 2^31 - 1; overlapping byte ranges of the two views (views that merely touch are fine); capacity * 20 * nframes or
 * capacity * 16 * nframes overflowing size_t; one frame's table above the scratch bound.  Every refusal lies above the first
 * allocation or launch.  Measurements: profiles/ccl/README.md. */
enum { HC_CC_STAT_LEFT = 0, HC_CC_STAT_TOP, HC_CC_STAT_WIDTH, HC_CC_STAT_HEIGHT, HC_CC_STAT_AREA, HC_CC_STAT_WORDS };
int hc_connected_components_device(hc_ctx *ctx, const void *d_map, size_t pitch, size_t frame_stride, int nframes, int connectivity,
                                   void *d_labels, size_t label_pitch, size_t label_frame_stride,
                                   void *d_counts    /* uint32  [nframes] */,
                                   void *d_stats     /* int32   [nframes][capacity][5]; may be NULL when capacity == 0 */,
                                   void *d_centroids /* float64 [nframes][capacity][2]; may be NULL when capacity == 0 */,
                                   size_t capacity);

/* cv::erode, cv::dilate and cv::morphologyEx(MORPH_OPEN / MORPH_CLOSE / MORPH_GRADIENT) for CV_8U frames on the device -- the step
 * between cv::Canny and a labelling or outlining of its map: Canny contours are one pixel wide and break at junctions, so callers
 * close the map first (k_morph8: cudacam_amd/csrc/morph.hip).  The semantics are stated here and restated in tests/morph_ref.py
 * (numpy); like the rest of Mode O they are not pinned against a build of OpenCV.
 * Element: K x K with K = ksize in {3, 5, 7}, anchored at its centre.  `spans` points to K int8 half-widths in HOST memory (read
 *   before the call returns): row j (0 .. K-1) of the element covers the columns -spans[j] .. +spans[j] around the anchor, and
 *   spans[j] = -1 is an empty row.  Every span lies in -1 .. K/2 and at least one row is not empty.  That covers the three shapes
 *   of cv::getStructuringElement (the host function below) and every other element whose rows are convex and symmetric in x; the
 *   rows need not be symmetric in y.  Arbitrary masks are not offered.
 * Operation, per pixel and channel (the channels of 3-channel frames are independent and stay interleaved):
 *     dilate: out(y, x) = max over the rows j and dx in -spans[j] .. spans[j] of src(y + j - K/2, x + dx)
 *     erode:  the same with min
 *   The element is not reflected: that is cv::dilate / cv::erode.  HC_MORPH_OPEN = dilate(erode(src)), HC_MORPH_CLOSE =
 *   erode(dilate(src)), HC_MORPH_GRADIENT = dilate(src) - erode(src), saturated at 0 as cv::morphologyEx subtracts (the difference is
 *   negative only where the window holds no position of the frame, see the border rule: 0 there); each stage is an operation on
 *   whole frames under the border rule below, as cv::morphologyEx runs them.
 * Border: cv::erode / cv::dilate's default, BORDER_CONSTANT with morphologyDefaultBorderValue: positions outside the frame never
 *   take part.  A window with no position inside the frame gives 0 (dilate) or 255 (erode).  There is no other border mode.
 * Channels: `channels` is 1 or 3 (interleaved) and is the caller's, not the context's: edge maps have one channel on every context.
 *   channels = 3 needs a 3-channel context.  With channels = 1, nframes may reach the output frames of a max_batch run (max_batch,
 *   3 * max_batch with HC_OPT_PER_CHANNEL), as for hc_edge_points_device; with channels = 3 it is at most max_batch.
 * Views, as hc_gaussian_blur_device: u8 rows of channels * width bytes with any alignment of base, pitch and frame stride; no
 *   byte outside [row, row + channels * width) of a row is read or written on either side; height * pitch >= 2^32 on either side
 *   is HC_E_ARG; byte ranges that overlap are refused, ranges that merely touch are fine.
 * Asynchronous on the context stream (hc_set_stream honoured), in order with everything else queued there: behind hc_canny_device
 *   and ahead of hc_connected_components_device it needs no synchronisation.  It is not a run, exactly as hc_gaussian_blur_device
 *   is none (hc_last_run_info, the stage timers, the hysteresis schedule / history and the pipeline slots stay as they were), and
 *   like that entry it completes first a pipelined run still in flight whose output overlaps either view.
 * Scratch: HC_MORPH_ERODE, HC_MORPH_DILATE and HC_MORPH_GRADIENT use none (the gradient is two launches, the second subtracting
 *   in place).  HC_MORPH_OPEN and HC_MORPH_CLOSE keep the frames between their two stages in one buffer the context owns
 *   (allocated on first use, grown when a call needs more, freed by hc_destroy; rows padded to a multiple of 4 bytes), under the
 *   bound of hc_hough_lines_device's scratch (256 MiB): a batch that does not fit runs in passes of as many whole frames as do, and
 *   a single frame above the bound is HC_E_ARG.  Successive calls share it and are ordered by the stream they are queued on, as for
 *   hc_edge_points_device.
 * HC_E_ARG: a null pointer; channels not 1 or 3, or 3 on a one-channel context; op outside the enum; ksize not in {3, 5, 7}; a
 * span outside -1 .. K/2, or all rows empty; a pitch < channels * width; nframes out of range; nframes > 1 with a frame stride
 * smaller than height * pitch; height * pitch >= 2^32; overlapping views; a frame of intermediate results above the scratch bound.
 * Every refusal lies above the first allocation or launch.  Measurements: profiles/morph/README.md. */
enum { HC_MORPH_ERODE = 0, HC_MORPH_DILATE = 1, HC_MORPH_OPEN = 2, HC_MORPH_CLOSE = 3, HC_MORPH_GRADIENT = 4 };
enum { HC_MORPH_RECT = 0, HC_MORPH_CROSS = 1, HC_MORPH_ELLIPSE = 2 };
int hc_morphology_device(hc_ctx *ctx, const void *d_in, size_t in_pitch, size_t in_frame_stride, void *d_out, size_t out_pitch,
                         size_t out_frame_stride, int nframes, int channels, int op, int ksize, const int8_t *spans /* host, ksize values */);

/* The half-widths of cv::getStructuringElement(shape, Size(ksize, ksize)) for the entry above, on the host (no context, no GPU),
 * restated; not pinned against a build of OpenCV.  With K = ksize (3, 5, 7) and r = K / 2:
 *   HC_MORPH_RECT:    every span is r.
 *   HC_MORPH_CROSS:   r in the centre row, 0 in the others.
 *   HC_MORPH_ELLIPSE: spans[j] = nearbyint(r * sqrt((r * r - (j - r) * (j - r)) / (r * r))) in double: [0 1 0] (the cross),
 *                     [0 2 2 2 0] and [0 2 3 3 3 2 0].
 * HC_E_ARG: spans null; a shape outside the enum; ksize not in {3, 5, 7}.  A refusal writes nothing. */
int hc_structuring_element(int shape, int ksize, int8_t *spans);

/* The exact Euclidean distance transform of u8 maps on the device: for every pixel the distance to the nearest feature pixel,
 * and which pixel that is -- cv::distanceTransform(255 - edges, DIST_L2, DIST_MASK_PRECISE) with DIST_LABEL_PIXEL labels, the
 * per-pixel product callers take from an edge map: chamfer matching, watershed markers, snapping to the nearest contour
 * (k_dt_cols, k_dt_rows: cudacam_amd/csrc/dist.hip).  The semantics are stated here and restated in tests/dist_ref.py (numpy: a
 * brute force over all feature pixels, and a separable form); like the rest of Mode O they are not pinned against a build of
 * OpenCV.  DIST_L2 only.  With W, H the context's frame size:
 * Map.  d_map is what hc_connected_components_device reads: one-channel u8 maps of W x H in a pitched view, whatever `channels`
 *   the context has; any alignment of base, pitch and frame stride; pitch >= W; no byte outside [row, row + W) of a row is read.
 *   The map is never written.  target = HC_DT_TO_NONZERO: the feature pixels are the non-zero bytes -- "distance to the nearest
 *   edge": the 255 of a final map, the 128 / 255 of an HC_STAGE_THRESH map and a 1 alike.  target = HC_DT_TO_ZERO: the feature
 *   pixels are the zero bytes, cv::distanceTransform's own convention, which saves the caller an inversion pass.
 * Distance.  For pixel (x, y), d2 = the minimum over the frame's feature pixels (x', y') of (x - x')^2 + (y - y')^2, an exact
 *   integer: 0 on a feature pixel, HC_DT_NONE in every pixel of a frame without a feature pixel.  Frames are independent.
 *   dist_type = HC_DT_SQUARED_I32: d_dist receives d2 as int32 [H][W].  dist_type = HC_DT_F32: d_dist receives float32
 *   sqrtf((float)d2) -- one conversion of the int32 to float32, round to nearest even, then one correctly rounded IEEE square
 *   root -- and +inf where d2 == HC_DT_NONE.  (From d2 > 2^24 on, which frames of 4100 columns reach, the conversion rounds, and
 *   the result is not always the float nearest to the square root taken in double: d2 = 6145^2 + 2^2 = 37,761,029 is the first
 *   example a single feature pixel at a corner gives, d2 = 77,632,802 another.)
 * Nearest.  When d_nearest is not null it receives, as int32 [H][W], the index y' * W + x' of a nearest feature pixel, and -1 in
 *   every pixel of a frame without one.  Among the feature pixels at distance d2 it is the one with the smallest x', and among
 *   those the one with the smallest y'.  That is the information of cv::distanceTransform's `labels` with DIST_LABEL_PIXEL, as
 *   coordinates instead of OpenCV's running numbers.
 * Output views, as the label plane of hc_connected_components_device: dist_pitch, dist_frame_stride, nearest_pitch and
 *   nearest_frame_stride in bytes; base, pitch and frame stride multiples of 4; pitch >= 4 * W.  Exactly the bytes
 *   [row, row + 4 * W) of every row are written, so either may be an ROI of a larger plane.  While the call runs the planes hold
 *   intermediate values.  nearest_pitch and nearest_frame_stride are not looked at when d_nearest is null.  No two of the three
 *   views may overlap, by the rule of the other entries: the byte ranges from a view's first to its last byte must not meet
 *   (ranges that merely touch are fine).  One exception: d_dist and d_nearest may be ROIs of one plane side by side -- equal
 *   pitches, equal frame strides (nframes > 1), bases at least 4 * W and at most pitch - 4 * W bytes apart -- whose ranges
 *   interleave without sharing a byte.
 * Asynchronous on the context stream (hc_set_stream honoured); chained behind hc_canny_device or hc_morphology_device it needs no
 * synchronisation.  Contexts of either mode.  It is not a run, exactly as hc_connected_components_device is none
 * (hc_last_run_info, the stage timers, the hysteresis schedule / history and the pipeline slots stay as they were), and like
 * that entry it completes first a pipelined run still in flight whose output overlaps any of the three views.
 * No scratch, no allocation, no passes, no atomics: between the two kernels the distance plane itself holds, per pixel, the
 * vertical offset to the nearest feature pixel of its column.  The result is a function of the map alone.
 * HC_E_ARG: ctx, d_map or d_dist null; target or dist_type outside its enum; pitch < W; an output base, pitch or frame stride
 * that is no multiple of 4; an output pitch < 4 * W; H * pitch >= 2^32 on any side; nframes outside 1..(max_batch, 3 * max_batch
 * with HC_OPT_PER_CHANNEL) or above 65535; nframes > 1 with a frame stride below H * pitch on any side; a view that wraps the
 * address space; any two of the views overlapping (views that merely touch are fine); W * H >= 2^31 - 1; (W - 1)^2 + (H - 1)^2
 * >= 2^31 - 1; W > 16384 (k_dt_rows keeps a row of W int32 in LDS).  Every refusal lies above the first launch, and a refused call
 * writes nothing.  Measurements: DESIGN.md 3.7k (tools/dist_bench.py). */
enum { HC_DT_TO_NONZERO = 0, HC_DT_TO_ZERO = 1 };          /* which pixels are the features */
enum { HC_DT_SQUARED_I32 = 0, HC_DT_F32 = 1 };             /* what d_dist receives */
#define HC_DT_NONE 2147483647                               /* squared distance of a frame without a feature pixel */
int hc_distance_transform_device(hc_ctx *ctx, const void *d_map, size_t pitch, size_t frame_stride, int nframes, int target, int dist_type,
                                 void *d_dist, size_t dist_pitch, size_t dist_frame_stride,
                                 void *d_nearest /* may be NULL */, size_t nearest_pitch, size_t nearest_frame_stride);

/* Thinning of binary maps on the device: the Zhang-Suen and the Guo-Hall skeleton, what callers take from
 * cv::ximgproc::thinning(.., THINNING_ZHANGSUEN / THINNING_GUOHALL) -- the inverse step of hc_morphology_device: a closed edge map
 * has contours three to seven pixels wide, and the point lists, Hough transforms and distances that follow want them one pixel
 * wide again (k_thin_pack, k_thin_step, k_thin_unpack: cudacam_amd/csrc/thin.hip, on bit planes, one bit per pixel).  The
 * semantics are stated here and restated in tests/thin_ref.py (numpy, and a naive per-pixel loop); like the rest of Mode O they
 * are not pinned against a build of OpenCV.  With W, H the context's frame size:
 * Map.  d_map is what hc_connected_components_device reads: one-channel u8 maps of W x H in a pitched view, whatever `channels`
 *   the context has; any alignment of base, pitch and frame stride; pitch >= W; no byte outside [row, row + W) of a row is read.
 *   A pixel is foreground iff its byte is non-zero.  Frames are independent.  The map is never written.
 * Neighbours.  For pixel P1 at (y, x) the eight neighbours are numbered clockwise from north: P2 (y-1, x), P3 (y-1, x+1),
 *   P4 (y, x+1), P5 (y+1, x+1), P6 (y+1, x), P7 (y+1, x-1), P8 (y, x-1), P9 (y-1, x-1); each is 1 for foreground and 0 otherwise,
 *   and a position outside the frame is background.  Every pixel of the frame, its outermost rows and columns included, is a
 *   candidate: the textbook rule.  (opencv_contrib's implementation, as far as it is remembered here and not checked, leaves the
 *   outermost rows and columns as they are; a caller who compares with it should look there first.)
 * Sub-iteration s (0 or 1), method = HC_THIN_ZHANGSUEN.  B = P2 + .. + P9; A = the number of positions i in the cyclic sequence
 *   P2, P3, .., P9, P2 with P_i = 0 and P_(i+1) = 1.  A foreground pixel is removed iff 2 <= B <= 6, A == 1 and
 *   s = 0: P2 P4 P6 == 0 and P4 P6 P8 == 0;   s = 1: P2 P4 P8 == 0 and P2 P6 P8 == 0.
 * Sub-iteration s, method = HC_THIN_GUOHALL.  C = (!P2 & (P3 | P4)) + (!P4 & (P5 | P6)) + (!P6 & (P7 | P8)) + (!P8 & (P9 | P2));
 *   N1 = (P9 | P2) + (P3 | P4) + (P5 | P6) + (P7 | P8); N2 = (P2 | P3) + (P4 | P5) + (P6 | P7) + (P8 | P9); N = min(N1, N2);
 *   m = (P6 | P7 | !P9) & P8 for s = 0 and (P2 | P3 | !P5) & P4 for s = 1.  A foreground pixel is removed iff C == 1,
 *   2 <= N <= 3 and m == 0.
 * Parallel rule.  All decisions of a sub-iteration are taken on the map as it was when the sub-iteration began; the removed
 *   pixels are cleared together.  (Zhang-Suen therefore erases an isolated 2 x 2 block; Guo-Hall leaves one pixel of it.)
 * Iterations.  Iteration k = 1, 2, .. is sub-iteration 0 followed by sub-iteration 1, and r_k the number of pixels it removes.
 *   An iteration depends on nothing but the map it starts from, so r_k = 0 means the map is a fixed point.  Let K be the smallest
 *   k <= max_iterations with r_k = 0, if there is one.  The output is the map after min(K - 1, max_iterations) iterations, written
 *   as 0 / 255.  A call with max_iterations too small returns exactly that intermediate map, and a second call on its output goes
 *   on from there and ends at the same fixed point.
 * Output view.  Exactly the bytes [row, row + W) of each row of each frame are written; base, pitch and frame stride may have any
 *   alignment (4-byte aligned views get dword stores); out_pitch >= W.  The byte ranges of the two views, from a view's first to
 *   its last byte, must not overlap (there is no in-place operation); ranges that merely touch are fine.
 * Status.  When d_status is not null (4-byte aligned) it receives uint32 [nframes][2]: d_status[f][0] = the number of iterations
 *   of frame f that removed a pixel (K - 1, or max_iterations), d_status[f][1] = 1 iff K exists, that is, the output is known to be
 *   the fixed point.  Nothing else is written.
 * Asynchronous on the context stream (hc_set_stream honoured); chained behind hc_morphology_device and ahead of
 *   hc_edge_points_device or hc_connected_components_device it needs no synchronisation.  Contexts of either mode.  It is not a
 *   run, exactly as hc_morphology_device is none (hc_last_run_info, the stage timers, the hysteresis schedule / history and the
 *   pipeline slots stay as they were), and like that entry it completes first a pipelined run still in flight whose output
 *   overlaps either view.
 * Scratch.  Owned by the context, allocated on first use, grown when a call needs more, freed by hc_destroy: per frame of a pass
 *   two bit planes (H rows of ceil(W / 32) dwords each) and a table of max_iterations + 1 removal words, under the bound of
 *   hc_hough_lines_device's scratch (256 MiB).  A batch that does not fit runs in passes of as many whole frames as do, and a
 *   single frame above the bound is HC_E_ARG.  Successive calls share it and are ordered by the stream they are queued on, across
 *   a change of the stream too.
 * Cost.  Every one of the 2 * max_iterations sub-iteration launches of a pass is queued whatever the content; the waves of a frame
 *   that has reached its fixed point exit on their first load, and the removal counts are integer sums, so the result is a function
 *   of the map alone.  max_iterations is therefore a cost, and 16 suits closed Canny maps: the largest count the restatement
 *   needed on 3 x 3-dilated curves is 7 (Guo-Hall), and the closed 1080p Canny maps of the eight synthetic scenes that
 *   tools/thin_bench.py measures -- no more than those eight -- needed at most 10 (Zhang-Suen).  Thick blobs take more, about
 *   half their thickness, and the continuation above serves them.
 *   Measurements: DESIGN.md 3.7l, profiles/thinning/README.md (tools/thin_bench.py).
 * HC_E_ARG: ctx, d_map or d_out null; method outside the enum; max_iterations outside 1..1024; d_status not 4-byte aligned;
 * pitch < W on either side; H * pitch >= 2^32 on either side; nframes outside 1..(max_batch, 3 * max_batch with
 * HC_OPT_PER_CHANNEL); nframes > 1 with a frame stride below H * pitch; a view that wraps the address space; overlapping views;
 * one frame's scratch above the bound.  Every refusal lies above the first allocation or launch, and a refused call writes
 * nothing. */
enum { HC_THIN_ZHANGSUEN = 0, HC_THIN_GUOHALL = 1 };
int hc_thinning_device(hc_ctx *ctx, const void *d_map, size_t pitch, size_t frame_stride, void *d_out, size_t out_pitch,
                       size_t out_frame_stride, int nframes, int method, int max_iterations,
                       void *d_status /* uint32 [nframes][2]; may be NULL */);

/* Corners on the device, the other half of a feature front end: the Harris / smallest-eigenvalue measure of given derivatives
 * (cv::cornerHarris / cv::cornerMinEigenVal, cv::cuda::createHarrisCorner / createMinEigenValCorner) and the strong, well-separated
 * local maxima of a response plane (cv::goodFeaturesToTrack, cv::cuda::createGoodFeaturesToTrackDetector), chained like the edge
 * points and the Hough entries (cudacam_amd/csrc/corners.hip).  The semantics are stated here and restated in tests/corner_ref.py
 * (numpy); like the rest of Mode O they are the library's own statement, not pinned against a build of OpenCV, and every deviation
 * from OpenCV is named: border, units, interior rule, capacity.  W, H: the context's frame size.
 *
 * hc_corner_response_device.
 * Input.  d_dx, d_dy: ONE-channel int16 planes of W x H with a common pitch and frame stride (bytes), exactly what
 *   hc_derivatives_device writes on a 1-channel context, at any ksize; any int16 value is legal, -32768 included.  Nothing of the
 *   input is written.
 * Window.  block_size B is 3, 5 or 7, centred; window positions are clamped to the frame (replicate), as the derivative entry
 *   clamps.  DEVIATION (border): OpenCV's box filter reflects (BORDER_REFLECT_101 by default), so the results differ from OpenCV's
 *   in the outermost B / 2 rows and columns -- on top of what the derivatives' own border does.
 * Sums.  Over the B x B window a = sum dx^2, b = sum dx dy, c = sum dy^2, as EXACT integers (they do not fit 32 bits: 49 * 2^30 at
 *   most); the order of summation cannot matter.
 * Response.  fa = (float)a, fb = (float)b, fc = (float)c, each one conversion of the exact integer, round to nearest even.  Every
 *   step below is one rounded float32 operation, the root correctly rounded:
 *   HC_CORNER_MIN_EIGEN: h = 0.5f fa, g = 0.5f fc, d = h - g; r = (h + g) - sqrtf(d d + fb fb).
 *   HC_CORNER_HARRIS:    k = (float)harris_k, t = fa + fc;    r = (fa fc - fb fb) - (k t) t.
 *   DEVIATION (units): there is no normalisation; values are in derivative^2 (min-eigen) or derivative^4 (Harris) units.
 *   OpenCV scales the derivatives of aperture ksize by s = 1 / (255 * 2^(ksize-1) * B) first, so its values are s^2 (min-eigen) or
 *   s^4 (Harris) times these; quality_level below is relative, so the corner selection does not depend on the factor.
 * Memory.  No byte outside [row, row + 2 W) of an input row is read, none outside [row, row + 4 W) of an output row is written;
 *   both sides may be ROIs of larger planes.  Alignment: d_dx, d_dy, pitch, frame_stride even; d_response, out_pitch,
 *   out_frame_stride multiples of 4; wider alignment (8 on the input, 8 / 16 on the output) gets wider accesses.  Offsets are
 *   32-bit: H * pitch and H * out_pitch must be below 2^32.
 * Asynchronous on the context stream (hc_set_stream honoured); behind hc_derivatives_device and ahead of hc_good_features_device
 *   it needs no synchronisation.  Contexts of either mode and any `channels`: the planes have one channel.  It is not a run,
 *   exactly as hc_derivatives_device is none.  No scratch.
 * HC_E_ARG: ctx, d_dx, d_dy or d_response null; misalignment; pitch < 2 W, out_pitch < 4 W; H * pitch or H * out_pitch >= 2^32;
 * nframes outside 1..(max_batch, 3 * max_batch with HC_OPT_PER_CHANNEL), the bound of hc_hough_circles_device; nframes > 1 with a
 * frame stride below H * pitch; a view that wraps the address space; block_size not 3, 5, 7; method outside the enum; harris_k not
 * finite with HC_CORNER_HARRIS (it is ignored with HC_CORNER_MIN_EIGEN); the byte range of the response view overlapping that of
 * either derivative plane.  Every refusal lies above the launch, and a refused call writes nothing. */
enum { HC_CORNER_MIN_EIGEN = 0, HC_CORNER_HARRIS = 1 };
int hc_corner_response_device(hc_ctx *ctx, const void *d_dx, const void *d_dy, size_t pitch, size_t frame_stride /* int16, ONE channel */,
                              void *d_response, size_t out_pitch, size_t out_frame_stride /* float32, W x H */,
                              int nframes, int block_size, int method, double harris_k);

/* hc_good_features_device: cv::goodFeaturesToTrack on a float32 response plane of W x H -- the form of cv::cuda::CornersDetector, a
 * function of the plane alone; the plane may be the caller's own, and nothing of it is written.  Frames are independent.
 * Keys.  key(v) = the bits of v as uint32 if v > 0.0f, else 0: NaN, -0 and negatives give 0, denormals keep their bits, +inf
 *   orders above every finite value.  All comparisons below are on keys, so they are integer comparisons.
 * Threshold.  M is the value with the largest key among ALL W * H pixels of the frame; q = (float)quality_level; t = M q, one
 *   rounded product.  A pixel passes iff key(v) > key(t).  M with key 0 gives no corners (and so does M = +inf).
 * Candidates.  A passing pixel with 1 <= x <= W - 2 and 1 <= y <= H - 2 whose key is >= the keys of all eight neighbours:
 *   OpenCV's val == dilate(val), on the interior.  DEVIATION (interior rule): the outermost rows and columns count for M and as
 *   neighbours but are never corners; frames with W < 3 or H < 3 have none.  A plateau makes every one of its pixels a candidate.
 * Order and cut.  Key descending, ties by ascending index y W + x.  Only the first candidate_capacity (1 .. 4096) candidates in that
 *   order go on.  DEVIATION (capacity): cv::goodFeaturesToTrack sifts all of them; this is the analogue of the centre cut of
 *   hc_hough_circles_device, and the one way the kept set can differ from OpenCV's rule on the same plane.
 * Smallest distance.  min_d2 = ceil(min_distance * min_distance), the product as a double -- the smallest int64 whose double is >=
 *   it --, capped at 2^62 as in hc_hough_circle_geometry; min_distance 0 gives 0.  The candidates are gone through in that order,
 *   and one is kept iff every candidate kept before it lies at squared distance >= min_d2 (int64 arithmetic).
 * Output.  d_corner_counts[f] is the full number kept, always.  The slot of frame f (corner_capacity corners) receives its first
 *   min(count, corner_capacity) corners as ((float)x, (float)y): the memory of a CV_32FC2 / std::vector<cv::Point2f>.  With
 *   d_quality, slot f of it (corner_capacity floats) receives their response values bit for bit.  corner_capacity 0 gives the
 *   counts only.  Nothing else is written.
 * Asynchronous on the context stream (hc_set_stream honoured); not a run, as hc_hough_circles_device is none.
 * Scratch.  Owned by the context, allocated on first use, grown when a call needs more, freed by hc_destroy: per frame of a pass
 *   40 bytes a candidate of capacity, a histogram of 2048 words, 8 state words and 2 words a row -- no plane --, under the bound of
 *   hc_hough_lines_device's scratch (256 MiB).  A batch that does not fit runs in passes of as many whole frames as do.  Successive
 *   calls share it and are ordered by the stream they are queued on, across a change of the stream too.
 * Cost.  Six walks over the plane (the maximum, three histogram passes of an exact radix select of the cut key -- digits of 11, 11
 *   and 10 bits --, a count and an emit in raster order), whatever the number of candidates; only the rank and the sift are
 *   quadratic, in candidate_capacity.  All sums are integer sums: the result is a function of the plane alone.
 * HC_E_ARG: ctx, d_response or d_corner_counts null, d_corners null with corner_capacity > 0; d_response, pitch or frame_stride not
 * multiples of 4, d_corner_counts or d_quality not 4-byte, d_corners not 8-byte aligned; pitch < 4 W; H * pitch >= 2^32; nframes > 1
 * with a frame stride below H * pitch; a view that wraps the address space; quality_level not finite or outside (0, 1];
 * min_distance not finite or negative; candidate_capacity outside 1..4096; nframes outside the bound above; corner_capacity * 8 *
 * nframes overflowing size_t; one frame's scratch above the bound.  Every refusal lies above the first allocation or launch. */
int hc_good_features_device(hc_ctx *ctx, const void *d_response, size_t pitch, size_t frame_stride /* float32, W x H */, int nframes,
                            double quality_level, double min_distance, size_t candidate_capacity,
                            void *d_corner_counts /* uint32 [nframes] */, void *d_corners /* float32 [nframes][corner_capacity][2] = (x, y) */,
                            void *d_quality /* float32 [nframes][corner_capacity], may be NULL */, size_t corner_capacity);

/* Sparse optical flow on the device: cv::pyrDown and one pyramid level of cv::calcOpticalFlowPyrLK, which follows the corner lists of
 * hc_good_features_device into the next frame (cudacam_amd/csrc/flow.hip).  The semantics are stated here and restated in
 * tests/flow_ref.py (numpy); like the rest of Mode O they are the library's own statement, not pinned against a build of OpenCV, and
 * every deviation from OpenCV is named.  Both entries take the size of the planes they work on PER CALL, because pyramid levels are
 * smaller than the context's W x H frame: 1 <= width <= W, 1 <= height <= H, plus the minimum each entry states.  The caller owns
 * every pyramid plane; neither entry has scratch.  Both are asynchronous on the context stream (hc_set_stream honoured) and are not
 * runs, as hc_corner_response_device is none; a pipelined run in flight whose output overlaps one of their u8 views is completed first,
 * as hc_morphology_device does.
 *
 * hc_pyr_down_device: cv::pyrDown(src, dst) for one-channel u8 planes of src_width x src_height.
 * Arithmetic.  dw = (src_width + 1) / 2, dh = (src_height + 1) / 2;
 *   dst(x, y) = (sum_{j=-2..2} sum_{i=-2..2} t[i] t[j] src(r(2x+i, src_width), r(2y+j, src_height)) + 128) >> 8, t = {1, 4, 6, 4, 1},
 *   r = BORDER_REFLECT_101 (-1 -> 1, -2 -> 2, n -> n-2, n+1 -> n-3).  All integer; the sum fits 16 bits.
 * Memory.  Any alignment on both sides, and both may be ROIs: no byte outside [row, row + src_width) of a source row is read, none
 *   outside [row, row + dw) of a destination row is written.  Offsets are 32-bit: height * pitch below 2^32 on both sides.
 * HC_E_ARG: ctx, d_src or d_dst null; src_width or src_height below 3 (one reflection suffices) or above the context's; pitch <
 * src_width, dst_pitch < dw; nframes outside the bound of hc_corner_response_device; nframes > 1 with frame_stride < src_height *
 * pitch or dst_frame_stride < dh * dst_pitch; offsets of 2^32 and more; a view that wraps the address space; overlapping byte ranges
 * of the two views.  Every refusal lies above the launch, and a refused call writes nothing. */
int hc_pyr_down_device(hc_ctx *ctx, const void *d_src, size_t pitch, size_t frame_stride, int src_width, int src_height,
                       void *d_dst, size_t dst_pitch, size_t dst_frame_stride, int nframes);

/* hc_lk_flow_device: ONE pyramid level of cv::calcOpticalFlowPyrLK on u8 planes of width x height (level `level` of both frames, with
 * one pitch and frame stride).  A full track is levels + 1 calls from the coarsest level down to level 0 on one stream with no
 * synchronisation between them: the first with use_initial as the caller has a guess or not, the others with use_initial 1.
 * d_counts and d_prev_pts are exactly what hc_good_features_device writes; min(counts[f], capacity) points of frame f are processed,
 * slots beyond that are not touched.  Points are (x, y) in LEVEL-0 units on both sides.
 * Every float step is one rounded float32 operation, none contracted; the root and the divisions are correctly rounded.
 *   s = 2^-level, S = 2^level (exact scalings); hw = (win - 1) * 0.5f.
 *   P(img, x, y) = img[clamp(y, 0, height-1)][clamp(x, 0, width-1)].
 *   Scharr on prev: Dx(x, y) = 3 (P(x+1,y-1) - P(x-1,y-1)) + 10 (P(x+1,y) - P(x-1,y)) + 3 (P(x+1,y+1) - P(x-1,y+1)), Dy its transpose:
 *   integers, |.| <= 4080.
 * 1. Weights at a position q = (qx, qy): ix = floorf(qx), a = qx - ix, iy, b likewise; t0 = 1 - a, t1 = 1 - b;
 *    w00 = (int)rintf((t0 t1) 16384), w01 = (int)rintf((a t1) 16384), w10 = (int)rintf((t0 b) 16384), w11 = 16384 - w00 - w01 - w10
 *    (rintf rounds half to even).  interp(F, i, j) = w00 F(ix+i, iy+j) + w01 F(ix+i+1, iy+j) + w10 F(ix+i, iy+j+1) + w11 F(ix+i+1, iy+j+1),
 *    an exact integer.
 * 2. q is OUT iff ix < -win or ix >= width or iy < -win or iy >= height, tested on ix, iy as floats before any conversion: NaN and
 *    values beyond int32 are out.
 * 3. Template.  u = prev_pts * s - hw.  u out: the point is LOST.  Otherwise, for 0 <= i, j < win, with arithmetic shifts:
 *    I(i, j) = (interp(P_prev) + 256) >> 9, gx(i, j) = (interp(Dx) + 8192) >> 14, gy likewise.
 * 4. Matrix.  A11 = sum gx^2, A12 = sum gx gy, A22 = sum gy^2 as exact int64; f11 = (float)A11 * 2^-20, f12, f22 likewise;
 *    D = f11 f22 - f12 f12; d = f11 - f22; m = (f22 + f11) - sqrtf(d d + 4 (f12 f12)); min_eig = m / (float)(2 win win).
 *    The point is lost iff min_eig < (float)min_eig_threshold or D < 1.1920929e-7f.  Dinv = 1.0f / D.
 * 5. Start.  v = (use_initial ? next_pts : prev_pts) * s - hw.
 * 6. For k = 0 .. max_iterations - 1: v out: the point is lost.  With the weights at v: diff(i, j) = ((interp(P_next) + 256) >> 9) -
 *    I(i, j); b1 = sum diff gx, b2 = sum diff gy as exact int64; g1 = (float)b1 * 2^-20, g2 likewise;
 *    ex = (f12 g2 - f22 g1) Dinv, ey = (f12 g1 - f11 g2) Dinv; v += e.  Stop if ex ex + ey ey <= (float)(epsilon * epsilon), the
 *    product taken as a double.  If k > 0 and |ex + px| < 0.01f and |ey + py| < 0.01f (p: the e of the iteration before):
 *    v -= e * 0.5f and stop.
 * 7. Not lost: next_pts = (v + hw) * S.  Lost: next_pts = (use_initial ? next_pts : prev_pts), bit for bit.
 * 8. Only with level == 0 are d_status and d_err written: status = 1 iff the point is not lost and the final v is not out, else 0.
 *    With d_err: status 1: diff recomputed at the final v, err = (float)(sum |diff|) / (float)(32 win win); status 0: err = 0.
 * DEVIATIONS from OpenCV: pixel fetches are clamped to the level (OpenCV pads its pyramid and takes derivatives of the padded
 * planes); the window sums are exact integers (OpenCV adds floats, in an order that depends on its vector width); a lost point stays
 * lost only for the level's call: the next level starts again from the unchanged position.
 * HC_E_ARG: the view rules of hc_pyr_down_device for both images (width, height >= 1); level outside 0..15; win even or outside
 * 5..31; max_iterations outside 1..64; epsilon or min_eig_threshold not finite or negative; capacity 0 or above 2^30 (a wave per
 * slot), or capacity * 8 * nframes overflowing size_t; a null pointer but d_err; d_counts, d_prev_pts, d_next_pts or d_err not 4-byte
 * aligned; d_next_pts overlapping d_prev_pts, d_counts or either image.  Every refusal lies above the launch. */
int hc_lk_flow_device(hc_ctx *ctx, const void *d_prev, const void *d_next, size_t pitch, size_t frame_stride /* u8 levels, common geometry */,
                      int width, int height, int level, int nframes,
                      const void *d_counts /* uint32 [nframes] */, const void *d_prev_pts /* float32 [nframes][capacity][2], level-0 units */,
                      void *d_next_pts /* float32, same shape, level-0 units, in/out */, size_t capacity,
                      int win /* odd, 5..31 */, int max_iterations /* 1..64 */, double epsilon, double min_eig_threshold, int use_initial,
                      void *d_status /* uint8 [nframes][capacity] */, void *d_err /* float32 [nframes][capacity], may be NULL */);

/* The hysteresis stage alone (kernels `hysteresis` + `removeCandidates`, src/cvp/cannyEdgeD.cu:295-395,
 * loop of cannyEdgeH.cu:297-338) on device tri-state maps (0 / 128 / 255) -> 0 / 255. */
int hc_hysteresis_device(hc_ctx *ctx, const void *d_thresh, size_t in_pitch, size_t in_frame_stride, void *d_out, size_t out_pitch,
                         size_t out_frame_stride, int nframes);

/* Device -> host copy of the output images of the last hc_run (the reference leaves them in the
 * GL PBO; a headless MI355X has no GL: this is the generalised sink). Synchronises. */
int hc_download(hc_ctx *ctx, uint8_t *host, size_t row_stride, size_t frame_stride, int nframes);

/* The same in two halves, for host pipelines that keep several contexts busy (cvp::io::FrameStreamer): _begin queues the
 * device -> host copy of the last run's output images behind that run and returns at once -- so that the copy engine
 * has this context's download queued while the host goes on to upload and start the next context's batch (PCIe carries
 * both directions at once: 48 GB/s each way on the GPU box against 54 / 56 one at a time) -- and _end waits for it,
 * verifies the run's convergence and, in the rare case the hysteresis had to be continued from the host, repeats the
 * copy.  `host` should be page-locked (hc_host_alloc); it must stay valid until _end returns. */
int hc_download_begin(hc_ctx *ctx, uint8_t *host, size_t row_stride, size_t frame_stride, int nframes);
int hc_download_end(hc_ctx *ctx);

/* Waits for the context stream; also completes the rare hysteresis continuation. */
int hc_sync(hc_ctx *ctx);

/* Run on the caller's HIP stream instead of the context's own: `hip_stream` is a hipStream_t handle, and 0 / NULL
 * means what it means to HIP -- the device's null (legacy default) stream, which is also what
 * torch.cuda.current_stream().cuda_stream is unless the caller switched streams.  Front kernels, uploads and
 * (outside pipelined mode) the hysteresis are then queued on that stream, in order with the caller's own work on
 * it: a run sees everything queued before it.  The context's own stream is created non-blocking, i.e. it does NOT
 * synchronise with the null stream; hc_use_own_stream() goes back to it.  Either switch orders the incoming stream behind
 * everything queued on the outgoing one at the time of the switch -- the context's work and the caller's own alike -- by an
 * event, without waiting on the host: a run after the switch sees the frames of an hc_upload made before it, with and
 * without HC_OPT_COPY_STREAMS, and device-op entries that share a context's scratch stay in order across it. */
int hc_set_stream(hc_ctx *ctx, void *hip_stream);
int hc_use_own_stream(hc_ctx *ctx);

/* Replaces enableKernelProfiling / _startCudaTimer / _endCudaTimer (cannyEdgeH.hpp:31-32,
 * cannyEdgeH.cu:409-430): when enabled, hc_run brackets every kernel with hipEvents; after hc_sync,
 * hc_stage_time_ms returns the last profiled run's time attributed to `stage`, or -1 when that run did not execute the
 * stage (final_stage below it, or stage 0 on 1-channel input) -- book a sample only for times >= 0, as the reference
 * books a stage only when it ran.  Attribution: the plain per-stage kernels behind final_stage < HYSTER each have their
 * own interval.  On the HYSTER fast path one kernel covers several reference stages and has no internal boundary to
 * time: k_blur covers MONO (3-channel input) + GAUSSIAN, k_nms covers GRADIENT + NMS + THRESH, a fused front kernel
 * covers all of them, k_front_o (mode O) GRADIENT + NMS + THRESH, as does k_front_o_ext at apertures 5, 7 and -1 (HC_FORM_O_APERTURE5 / _APERTURE7 / _SCHARR);
 * on given gradients (hc_run_gradients_device, HC_FORM_O_GRADIENTS) it covers NMS + THRESH and GRADIENT reads -1; a kernel's time is divided EQUALLY among the stages
 * it covers, so every stage that ran shows a non-zero share and the sum over stages -- what the reference's UI totals
 * up to the selected stage (src/imgui/imguiApp.cpp:364-376) -- is the measured time.  Off by default on the batch path. */
int hc_enable_profiling(hc_ctx *ctx, int on);
int hc_stage_time_ms(hc_ctx *ctx, int stage, float *ms);
/* Sums over every profiled run since the last reset (up to 256 runs may be in flight between
 * syncs): sum_ms[0] stage 0, [1] fused front kernel (or the tap kernels), [2] hysteresis + expand.
 * This is the accumulating counterpart of timerManager::addTime (src/utils/timer.hpp:27-39). */
int hc_profile_get(hc_ctx *ctx, double sum_ms[3], long *nruns, int reset);
/* The front path's two kernels separately, over the same profiled runs (those that took the split path):
 * sum_ms[0] k_blur, [1] k_nms.  Read it before hc_profile_get(..., reset = 1), which clears both. */
int hc_profile_get_front(hc_ctx *ctx, double sum_ms[2], long *nruns);

/* Steady-state step times: for every pair of consecutive profiled runs since the last reset, the time from the end of
 * one run (its last kernel, hysteresis included) to the end of the next, in ms.  In pipelined mode, where runs overlap,
 * this -- not a run's own start-to-end time -- is what a frame stream sees.  Writes up to `cap` values, *n = how many exist. */
int hc_profile_get_intervals(hc_ctx *ctx, float *ms, int cap, int *n);

/* The front kernels' own time (ms) of every profiled HYSTER run since the last reset, in run order: what bench.py needs
 * to attribute kernel time to the content of each step when the batches of a stream differ.  Writes up to `cap` values,
 * *n = how many exist. */
int hc_profile_get_front_each(hc_ctx *ctx, float *ms, int cap, int *n);

/* Internal device buffers (input frames, output images) and their pitch / frame stride. */
int hc_device_ptrs(hc_ctx *ctx, void **d_in, void **d_out, size_t *in_pitch, size_t *out_pitch, size_t *in_frame_stride,
                   size_t *out_frame_stride);

/* Number of hysteresis launches that did work in the last run, and whether the continuation ran. */
int hc_last_hysteresis_info(hc_ctx *ctx, int *launches_with_work, int *continued);

/* The same, summed over every run completed since the context was created (or since the last call with reset != 0):
 * totals[0] = runs, totals[1] = runs that needed the host-side continuation (each one a stall of a pipelined stream),
 * totals[2] = hysteresis launches that found work, totals[3] = hysteresis launches queued.  Completes pending runs. */
int hc_hysteresis_totals(hc_ctx *ctx, unsigned long long totals[4], int reset);

/* The schedule the most recent completed run got (diagnostics; read-only, changes nothing).  How a run's hysteresis is
 * queued follows what the earlier runs of the context observed; a prediction that is wrong costs time, never a pixel,
 * and this entry lets a test see which schedule it exercised.  Completes pending runs, then writes up to `nwords` of:
 *   info[HC_SCHED_LAUNCHES]    hysteresis launches queued (rounds, when the looping launch ran them)
 *   info[HC_SCHED_LISTS]       0 = a workgroup per tile in every launch, 1 = worklists from launch 1 on,
 *                              2 = mixed: a workgroup per tile first, lists from launch 3 on (launch 2 writes the first)
 *   info[HC_SCHED_LOOP]        1 = all rounds ran inside one looping launch (k_hyst_loop)
 *   info[HC_SCHED_HIST_GRID]   smallest grid of a list launch that was sized from the previous run's list lengths
 *                              (max(2048, 2 * previous length + 256), at most the tile count); 0 = no launch was
 *   info[HC_SCHED_LONGEST]     longest worklist a launch of the run had to serve (entries handed on included)
 *   info[HC_SCHED_OVERFLOWS]   list launches whose history-sized grid was smaller than their list (entries handed on)
 *   info[HC_SCHED_TILES]       workgroup tiles of the run (frames x row tiles x column panels)
 *   info[HC_SCHED_TILE_ROWS], info[HC_SCHED_WAVES]   rows per wave and waves per workgroup: a tile has rows x waves rows
 *   info[HC_SCHED_PANELS]      column panels (2048 columns each)
 *   info[HC_SCHED_FRAMES]      output frames of the run
 * LONGEST and OVERFLOWS describe the launches the run queued: they are taken before a host-side continuation, whose
 * later lists they do not show.  All zero before the first completed HYSTER run. */
enum { HC_SCHED_LAUNCHES = 0, HC_SCHED_LISTS, HC_SCHED_LOOP, HC_SCHED_HIST_GRID, HC_SCHED_LONGEST, HC_SCHED_OVERFLOWS, HC_SCHED_TILES,
       HC_SCHED_TILE_ROWS, HC_SCHED_WAVES, HC_SCHED_PANELS, HC_SCHED_FRAMES, HC_SCHED_WORDS };
int hc_last_hysteresis_schedule(hc_ctx *ctx, int *info, int nwords);

/* The front path of a run, as hc_last_run_info reports it: which kernel turned the frames into the STRONG / CANDIDATE bit
 * planes.  The values are part of the ABI. */
enum {
  HC_FORM_FRONT_O = -1,     /* Mode O: k_front_o (4 px per lane); also "no front kernel ran" (final stages below HYSTER) */
  HC_FORM_FRONT4 = 0,       /* Mode R, HC_OPT_FRONT_SPLIT 0: the 4-px fused k_front (libhipcanny_legacy.so) */
  HC_FORM_SPLIT = 1,        /* Mode R, HC_OPT_FRONT_SPLIT 1: k_blur + k_nms (libhipcanny_legacy.so) */
  HC_FORM_FRONT8 = 2,       /* Mode R, HC_OPT_FRONT_SPLIT 2: k_front8 */
  HC_FORM_FRONT8O = 3,      /* Mode O: k_front8o */
  HC_FORM_FRONT8_HALF = 4,  /* Mode R: k_front8 in its half-strip form (HC_OPT_FRONT_HALF) */
  HC_FORM_FRONT_MX = 5,     /* Mode R: k_front_mx (HC_OPT_FRONT_MX) */
  HC_FORM_O_APERTURE5 = 6,  /* Mode O: k_front_o_ext at HC_OPT_APERTURE 5 */
  HC_FORM_O_GRADIENTS = 7,  /* Mode O: k_front_o_ext on given gradients (hc_run_gradients_device) */
  HC_FORM_O_APERTURE7 = 8,  /* Mode O: k_front_o_ext's fused 7x7 Sobel (hc_canny_device, aperture 7) */
  HC_FORM_O_SCHARR = 9      /* Mode O: k_front_o_ext's fused Scharr derivatives (hc_canny_device, aperture -1) */
};

/* What the last hc_run / hc_run_device did with the caller's buffers -- no silent cliffs: *input_staged / *output_staged are
 * 1 when the frames went through the context's internal pitched buffers (an extra device-to-device copy each: pointer,
 * pitch or frame stride not a multiple of 4, 3-channel mode O rows without whole 12-byte groups, or an input view with
 * height * pitch >= 2^32), and *front_form is the front path that ran, one of the HC_FORM_* values above (Mode R:
 * HC_FORM_FRONT8 / HC_FORM_SPLIT / HC_FORM_FRONT4 are the HC_OPT_FRONT_SPLIT values 2 / 1 / 0; HC_FORM_FRONT_O also for
 * final stages below HYSTER).  Rows that do not hold whole 8-pixel groups (tight rows of a width that is not a multiple
 * of 8) are staged (*input_staged = 1) so that the 8-px kernels can run. */
int hc_last_run_info(hc_ctx *ctx, int *input_staged, int *output_staged, int *front_form);

/* Pipelined mode: how many runs of `nframes` frames the context may keep in flight (4 for small batches -- fewer
 * than 0.5 G pixels per run; big batches: 3 -- the context uses two slots, and a third while it sees the hysteresis of
 * a run outlast the front kernel of the next (frames of several thousand columns); 1 when HC_OPT_PIPELINE is off):
 * the number of output buffers a caller should rotate through so that no run has to wait for an older one that still
 * writes the same memory.  No reference counterpart
 * (the reference processes one frame per synchronous call, src/cvp/cannyEdgeH.cu:49-120). */
int hc_pipeline_depth(hc_ctx *ctx, int nframes);
/* ... and how many slots the ring of the most recent pipelined run had (2 / 3 / 4; 1 when HC_OPT_PIPELINE is off). */
int hc_pipeline_slots_in_use(hc_ctx *ctx);
/* Waves per workgroup of the most recent k_front8 launch: 4, 1 (HC_OPT_FRONT_WPB) or 3 (per-channel mode: one per channel). */
int hc_front_waves_per_workgroup(hc_ctx *ctx);

/* Diagnostics of the last run's queued hysteresis launches: 3 words per launch
 * (sweeps summed over tiles, max sweeps of a tile, tiles that did work). */
int hc_hysteresis_stats(hc_ctx *ctx, unsigned *stats, int nwords);

/* Tuning knobs: rows per front-path work item (0 = auto; k_front8 / k_front8o round it up to whole 6-row windows, 2 rows at
 * least; the 4-px Mode O kernels -- k_front_o, and k_front_o_ext in all its forms -- take any number of
 * rows from 1 to the frame height as it is; larger values mean one item per strip); hysteresis launches queued per run (0 = auto:
 * 6, or one more than the row tiles + column panels of a frame, or what the last runs needed + 4, at most 96; launches
 * after convergence exit at once, and
 * hc_sync continues from the host in the rare case the queue was too short -- non-monotone, serpentine edges). */
int hc_set_tuning(hc_ctx *ctx, int chunk_rows, int hyst_launches);

/* Options.  HC_OPT_NMS_SATURATE (default 0): the reference stores `min((unsigned char)gradVal, 255)`
 * (src/cvp/cannyEdgeD.cu:267), an out-of-range float->u8 cast for gradients 256..721.  0 = the
 * canonical Mode R reading: the value wraps mod 256 (integer min folds away, low byte stored).
 * 1 = min(g, 255): what the same source line yields when compiled by hipcc for gfx950.
 *
 * HC_OPT_PIPELINE (default 0): throughput mode for back-to-back batches.  1 = the front kernels of
 * run i+1 (on the context stream) overlap the hysteresis + expand of run i (second stream, second set
 * of bit planes).  The front kernels run in order with the caller's own work on the context stream, so a
 * run sees what the caller queued before it and the input may be reused by work queued after it; the OUTPUT
 * of a run is only guaranteed after hc_sync() (or hc_download).  Results are identical in both modes.  Hand
 * consecutive runs different output buffers -- two in turn for big batches, four for small ones (fewer than
 * 0.5 G pixels per run: there four runs are kept in flight, each hysteresis on a stream of its own, because a
 * step is otherwise the latency of the hysteresis' chain of launches).  A run whose output overlaps that of a run
 * still in flight waits for it, and if that is the previous run it still gives the exact map, but without the
 * provisional-map shortcut and a few percent slower.
 *
 * HC_OPT_PER_CHANNEL (default 0, 3-channel contexts only): 1 = instead of the reference's grey
 * conversion, run the detector on each channel separately (BASELINE config "three-channel,
 * per-channel Canny"): the interleaved input is read once per channel by adjacent work items and
 * every run produces 3 edge maps per input frame, output frame 3*f + ch (ch = byte position in the pixel).
 *
 * HC_OPT_FRONT_SPLIT (default 2, Mode R): which kernels form the front path (grey | blur | Sobel | NMS | thresholds).
 * 2 = k_front8: ONE kernel, 8 pixels per lane, no intermediate in HBM (falls back to 1 when an input row does not hold
 * whole 8-pixel groups, i.e. pitch < round_up(width, 8) * channels; and, while the option has not been set by the
 * caller, for big batches (0.1 G pixels or more per run) of narrow frames whose width fills the 248-column strips of
 * the 4-px kernels much better than the 496-column strips of k_front8: up to 248 columns and 497..744 (VGA)); 1 = k_blur + k_nms with a u8 blur plane between
 * them; 0 = k_front, the earlier 4-pixel fused kernel.  Results are identical; 0 and 1 are kept as independent
 * implementations for the parity tests.  Mode O contexts: 2 = k_front8o, the 8-pixel kernel (one-channel sources;
 * 3-channel sources and rows without whole 8-pixel groups use k_front_o), 0 or 1 = k_front_o, the 4-pixel kernel.
 *
 * HC_OPT_L2_GRADIENT (default 0, Mode O contexts): cv::Canny's `L2gradient` argument: magnitude dx^2 + dy^2
 * compared with the squared thresholds instead of |dx| + |dy|.
 *
 * HC_OPT_APERTURE (default 3, Mode O contexts): cv::Canny's `apertureSize`.  5 = Sobel(src, CV_16S, ksize 5, scale 1,
 * BORDER_REPLICATE): |dx|, |dy| <= 12240, the L1 magnitude up to 24480; thresholds, the 3-channel select, the tangent test
 * and NMS as at 3.  Runs k_front_o_ext (HC_FORM_O_APERTURE5; 1 or 3 channels; rows without whole 4-pixel groups are staged).
 * Any other value, and any mode R context, is HC_E_ARG; 7 and -1 (Scharr) are not offered as options (cv::Canny scales the
 * 7x7 Sobel and its thresholds to stay within int16): such callers chain hc_derivatives_device (ksize 7 / -1, which states
 * the scaling and what it means for the thresholds) with hc_run_gradients_device, or call hc_canny_device, which takes the
 * aperture (any of 3, 5, 7, -1) and cv::Canny's own thresholds per call and runs one fused kernel.  Mode O thresholds stay clamped to 0..32767 at every aperture (L1 thresholds above 32767
 * cannot be expressed).
 * Pipelined mode (HC_OPT_PIPELINE) gives exact maps on both k_front_o_ext forms (HC_FORM_O_APERTURE5 and HC_FORM_O_GRADIENTS); they write no provisional map,
 * so the hysteresis writes the whole output map of their runs. */
/*
 * HC_OPT_DEBUG_TAPS (default 0): parity-test diagnostics.  1 = every HC_STAGE_HYSTER run keeps a copy of what the
 * FAST path's front kernels produced -- the STRONG and CANDIDATE bit planes as they are handed to the hysteresis,
 * and the blur plane (Mode R) -- for hc_debug_tap().  Costs two plane copies per run; never set it when timing.
 *
 * HC_OPT_FRONT_HALF (default -1 = automatic, Mode R): the half-strip form of k_front8 for narrow frames -- a wave is two
 * independent half-waves of 240 columns each, and the (frame, half-strip) units of a run of rows are dealt to them in pairs
 * (640 columns: 1.5 waves per frame instead of 2).  -1 = when it needs fewer waves; 0 = never; 1 = whenever the buffers
 * allow it (parity tests).  hc_last_run_info reports it as HC_FORM_FRONT8_HALF.
 *
 * HC_OPT_FRONT_DENSE (default -1 = automatic, Mode R): k_front8's dense path -- a window of 6 rows that follows one in
 * which more than 512 of the wave's 768 half-lanes passed the low threshold (noise, texture) is processed by wave-wide
 * non-maximum suppression in registers instead of the queue and its batches, until a window counts fewer than 384.
 * 0 = never, 1 = every window (parity tests).  Same results either way.
 *
 * HC_OPT_COPY_STREAMS (default 0): host pipelines of several contexts (cvp::io::FrameStreamer).  1 = hc_upload and
 * hc_download_begin move their data on two copy streams that ALL such contexts of a device share -- one for host ->
 * device, one for device -> host -- tied to the context stream by events, instead of on the context stream itself.
 * Copies that share a stream with kernels do not overlap across contexts on this runtime (three contexts, 32 MiB
 * batches: 28 GB/s each way; with the two copy streams 40, with 64 MiB batches 47 of the 48 GB/s the link carries both
 * ways at once -- tools/experiments/pcie_raw2.hip).
 *
 * HC_OPT_FRONT_WPB (default -1 = automatic, Mode R, mono / BGR input): waves per workgroup of k_front8 in pipelined big
 * batches.  One-wave workgroups refill a retiring wave's slot at once and gain the front kernel 2-3 % beside the
 * hysteresis of the previous run -- which then needs 40 % more stream time.  Automatic: one wave once that hysteresis
 * ends more than 25 % of a front kernel's time before the front kernel it runs beside, four again below 3 % (smoothed,
 * from the runs' own events); small batches (fewer than 0.5 G pixels per run): one wave from 0.12 G pixels.  1 or 4 fixes it.  Same results either way; hc_front_waves_per_workgroup says what ran.
 *
 * HC_OPT_PIPELINE_SLOTS (default -1 = automatic): the ring of big pipelined batches.  Automatic: two slots, and a third
 * while the context sees the hysteresis of a run end after the front kernel of the next one (hc_pipeline_depth).
 * 2 or 3 fixes the ring.  Diagnostics / tests: 20 / 21 = the automatic rule, but told that every chain ends after /
 * before the next front kernel, which walks it through its transitions (2 -> 3 on trial after three runs, kept or given back after ten; 3 -> 2 after sixteen)
 * whatever the content.  Same results with every value.
 *
 * HC_OPT_FRONT_MX (default 0, Mode R, one-channel frames): 1 = k_front_mx, the front path whose two integer
 * contractions (the 5x5 Gaussian sum, the 3x3 Sobel sums) run on the matrix pipe as v_mfma_i32_32x32x32_i8 (strips of 216
 * columns, blocks of 16 rows), for every run that allows it (input pitch >= round_up(width, 4), height x pitch < 2^32
 * -- other input views are staged first, so every one-channel run does; pipelined mode: the provisional map needs
 * width % 8 == 0 and height x output pitch < 2^32, other runs go without it).  Same results bit for bit; hc_last_run_info reports HC_FORM_FRONT_MX; HC_OPT_FRONT_WPB 1 / 4
 * picks its workgroup size.  Opt-in: measured on the MI355X (profiles/r04/mx_experiments.md) it takes 14 % less time than
 * k_front8 alone (1.83 against 2.14 ms per 1024 camera-like 1080p frames), 3-5 % less beside the hysteresis of the batch
 * before (2.37-2.43 against 2.50 ms), and half as much again on frames full of candidates (iid noise: 7.7 against 5.1 ms),
 * for which it has no dense path. */
enum { HC_OPT_NMS_SATURATE = 1, HC_OPT_PIPELINE = 2, HC_OPT_PER_CHANNEL = 3, HC_OPT_FRONT_SPLIT = 4, HC_OPT_L2_GRADIENT = 5, HC_OPT_DEBUG_TAPS = 6, HC_OPT_FRONT_HALF = 7,
       HC_OPT_FRONT_DENSE = 8, HC_OPT_COPY_STREAMS = 9, HC_OPT_PIPELINE_SLOTS = 10, HC_OPT_FRONT_WPB = 11, HC_OPT_FRONT_MX = 12, HC_OPT_APERTURE = 13,
       /* test and diagnostic hooks (the library reads no environment variables): hysteresis launches >= 1 on a fixed grid with
        * worklists (-1: lists, default grid); the looping hysteresis launch of small runs off (0) / on; per-launch statistics for
        * tools/hyst_diag.py; hysteresis workgroup shape (rows x 100 + waves, 0 = by the rule); k_front8's dense-path thresholds;
        * the bound, in bytes, of hc_hough_lines_device's scratch (<= 0: the default of 256 MiB), so that a small batch takes several passes;
        * the angles per workgroup of k_hough_vote (measurements; capped by what LDS and numangle allow; <= 0: by the plan's rule) */
       HC_OPT_TEST_HYST_LATE_GRID = 100, HC_OPT_TEST_HYST_LOOP = 101, HC_OPT_TEST_HYST_DIAG = 102, HC_OPT_TEST_HYST_GEOM = 103,
       HC_OPT_TEST_DENSE_ENTER = 104, HC_OPT_TEST_DENSE_LEAVE = 105, HC_OPT_TEST_HOUGH_SCRATCH = 106, HC_OPT_TEST_HOUGH_ROWS = 107 };
int hc_set_option(hc_ctx *ctx, int option, int value);

/* The fast path's own intermediates of the last HC_STAGE_HYSTER run (HC_OPT_DEBUG_TAPS must have been set before it),
 * as tight-or-strided host u8 images, one per output frame:
 *   HC_TAP_BLUR       the Gaussian blur the front kernels computed (reference: gaussianFilter5x5 output,
 *                     src/cvp/cannyEdgeD.cu:72-118); Mode R only
 *   HC_TAP_THRESH     the double-threshold map 0 / 128 / 255 (doubleThreshold output, cannyEdgeD.cu:273-293) rebuilt
 *                     from the two bit planes: 255 = STRONG bit, 128 = CANDIDATE bit only
 * These are NOT the plain per-stage kernels behind hc_run(final_stage < HYSTER): they read back what k_blur / k_nms /
 * k_front / k_front_o wrote, so that the parity tests can check the fast path stage by stage. */
enum { HC_TAP_BLUR = 1, HC_TAP_THRESH = 2 };
int hc_debug_tap(hc_ctx *ctx, int what, uint8_t *host, size_t row_stride, size_t frame_stride, int nframes);

/* Page-locked host memory for frame staging: hc_upload / hc_download on such buffers are true asynchronous DMA
 * (the reference uploads from pageable cv::Mat memory with a blocking cudaMemcpy2D, cannyEdgeH.cu:136/144).
 * Used by cvp::io::FrameStreamer (include/cvp/frameIO.hpp).  NULL on failure. */
void *hc_host_alloc(size_t bytes);
void hc_host_free(void *p);

/* Device self-test of the cross-lane / packed-math primitives the kernels rely on. 0 = ok. */
int hc_selftest(int device);

const char *hc_last_error(void);
const char *hc_version(void);

#ifdef __cplusplus
}
#endif
#endif
