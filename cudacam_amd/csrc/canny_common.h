// canny_common.h -- shared declarations of the hipcanny device code and its host launcher.
// Hand-written for gfx950 (CDNA4, wave64).  Not a translation of the reference's CUDA kernels:
// see DESIGN.md for the layout (strips, chunks, bit planes) and for why each choice was made.
#pragma once
#include <hip/hip_runtime.h>
#include "canny_params.h"  // parameter blocks and the geometry the host plans with (plain C++)

namespace hc {

// ---- host-callable launchers (defined in canny_kernels.hip unless noted) ----------------------
hipError_t launch_selftest(u32 *d_result, hipStream_t s);
hipError_t check_gauss_coeffs(const float gk[25]);
hipError_t launch_front_o(const FrontParams &p, hipStream_t s);
hipError_t launch_front_o_ext(const FrontExtParams &p, hipStream_t s);  // front_o_ext.hip
hipError_t launch_deriv16(const DerivParams &p, hipStream_t s);  // deriv.hip: Sobel 3 / 5 / 7 and Scharr derivatives, u8 -> int16 dx / dy
// stats.hip (the product library only, as the launchers down to launch_connected_components: the test library defines none of them): frame
// histograms and the automatic thresholds of Mode O
hipError_t launch_hist256(const HistParams &p, hipStream_t s);  // p.hist must be zero when the kernel starts
hipError_t launch_auto_thr(const u32 *hist, int nframes, int rule, double param, int32_t *thr, hipStream_t s);  // hist [nframes][256] -> thr [nframes][2]
// edge_points.hip (the product library only): k_edge_count, k_edge_scan and, with p.capacity > 0, k_edge_emit
hipError_t launch_edge_points(const EdgePointsParams &p, hipStream_t s);
hipError_t launch_gauss8(const BlurParams &p, hipStream_t s);  // blur.hip (the product library only): separable Q8 smoothing filter, u8 -> u8
// hough.hip (the product library only): one pass of k_hough_vote, k_hough_peaks (count), k_hough_scan, k_hough_peaks (emit) and,
// with p.line_capacity > 0, k_hough_rank
hipError_t launch_hough(const HoughParams &p, hipStream_t s);
// ... and its peaks part alone (k_hough_peaks count, k_hough_scan, k_hough_peaks emit), on any padded accumulator of that layout
hipError_t launch_hough_peaks(const HoughParams &p, hipStream_t s);
// hough_segments.hip (the product library only): k_seg_count, k_seg_scan and, with p.seg_capacity > 0, k_seg_emit
hipError_t launch_hough_segments(const SegParams &p, hipStream_t s);
// hough_circles.hip (the product library only): one pass of k_circle_vote (p.accum must be zero when it starts), the peaks
// (launch_hough_peaks), k_circle_rank, k_circle_sift, k_circle_radii (count), k_circle_scan and, with p.circle_capacity > 0,
// k_circle_radii (emit)
hipError_t launch_hough_circles(const CircleParams &p, hipStream_t s);
// ccl.hip (the product library only): one pass of k_ccl_local, k_ccl_merge, k_ccl_flatten, k_ccl_scan, k_ccl_roots, k_ccl_number
// and, with p.capacity > 0, k_ccl_rows, k_ccl_stats and k_ccl_finish
hipError_t launch_connected_components(const CclParams &p, hipStream_t s);
hipError_t launch_morph8(const MorphParams &p, hipStream_t s);  // morph.hip (the product library only): one maximum / minimum filter launch, u8 -> u8
hipError_t launch_distance_transform(const DistParams &p, hipStream_t s);  // dist.hip (the product library only): k_dt_cols, then k_dt_rows
// thin.hip (the product library only): the map -> bit plane A; sub-iteration `sub` (0: A -> B, 1: B -> A) of iteration `iteration`
// (1 ..; its removals are added to word `iteration` of each frame's table, and frames whose word iteration - 1 is zero are left
// alone); plane A -> the 0 / 255 output view and the status pairs
hipError_t launch_thin_pack(const ThinPackParams &p, hipStream_t s);
hipError_t launch_thin_step(const ThinStepParams &p, int sub, int iteration, hipStream_t s);
hipError_t launch_thin_unpack(const ThinUnpackParams &p, hipStream_t s);
// corners.hip (the product library only): k_corner_response; one pass of the kernels of hc_good_features_device (p.hist and p.state
// must be zero when it starts)
hipError_t launch_corner_response(const CornerParams &p, hipStream_t s);
hipError_t launch_good_features(const FeatParams &p, hipStream_t s);
// flow.hip (the product library only): k_pyr_down8; k_lk_flow, one pyramid level of the tracker
hipError_t launch_pyr_down(const PyrParams &p, hipStream_t s);
hipError_t launch_lk_flow(const FlowParams &p, hipStream_t s);
#ifdef HC_LEGACY_FRONT  // legacy_front.hip: the round-1 front kernels of Mode R, built into libhipcanny_legacy.so only (parity tests)
hipError_t launch_front(const FrontParams &p, hipStream_t s);
hipError_t launch_blur(const FrontParams &p, hipStream_t s);
hipError_t launch_nms(const FrontParams &p, hipStream_t s);
size_t front_lds_bytes();
#endif
// front8.hip: the whole front path as one kernel, 8 px per lane (strips of 496 columns, runs of 6 * windows - 4 rows)
hipError_t launch_front8(const FrontParams &p, hipStream_t s);
hipError_t launch_front8o(const FrontParams &p, hipStream_t s);  // Mode O on the same skeleton (one-channel sources)
// front_mx.hip: Mode R, one-channel frames, the blur and Sobel contractions as i8 MFMAs (strips of 216 columns, runs of
// 16 * blocks rows); big batches
hipError_t launch_front_mx(const FrontParams &p, hipStream_t s);
hipError_t launch_hyst(const HystParams &p, hipStream_t s);  // hyst.hip, as the next two
// the first `rounds` launches of the workgroup-per-tile form as ONE launch with device-wide barriers between the rounds
// (small runs: at most HYST_LOOP_MAX_TILES tiles); bar: two zeroed words (arrival counter, abort flag)
hipError_t launch_hyst_loop(const HystParams &p, int rounds, u32 *bar, hipStream_t s);
hipError_t launch_pack(const PackParams &p, hipStream_t s);
// pitched device-to-device copy of n frames (any alignment on either side); rows, n <= 65535
hipError_t launch_copy_rows(void *dst, size_t dpitch, size_t dfs, const void *src, size_t spitch, size_t sfs, size_t row_bytes, int rows, int n, hipStream_t s);

// plain per-stage kernels (exact, unfused): the `finalStage` taps MONO..THRESH of CannyEdge::run
hipError_t launch_gray(const uint8_t *bgr, size_t bpitch, size_t bfs, uint8_t *mono, size_t mpitch, size_t mfs, int W, int H, int n, hipStream_t s);
hipError_t launch_gauss(const uint8_t *mono, size_t mpitch, size_t mfs, uint8_t *blur, size_t bpitch, size_t bfs, int W, int H, int n, hipStream_t s);
hipError_t launch_sobel(const uint8_t *blur, size_t bpitch, size_t bfs, int16_t *sx, int16_t *sy, size_t spitch_elems, size_t sfs_elems, int W, int H, int n, hipStream_t s);
hipError_t launch_graddisp(const int16_t *sx, const int16_t *sy, size_t spitch_elems, size_t sfs_elems, uint8_t *out, size_t opitch, size_t ofs, int W, int H, int n, hipStream_t s);
hipError_t launch_nms(const int16_t *sx, const int16_t *sy, size_t spitch_elems, size_t sfs_elems, uint8_t *out, size_t opitch, size_t ofs, int W, int H, int n, int saturate, hipStream_t s);
hipError_t launch_thresh(const uint8_t *nms, size_t npitch, size_t nfs, uint8_t *out, size_t opitch, size_t ofs, int W, int H, int n, int low, int high, hipStream_t s);

}  // namespace hc
