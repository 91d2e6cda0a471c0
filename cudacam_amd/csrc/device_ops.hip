// device_ops.hip -- the entry points of libhipcanny.so that are not runs: one or a few kernels on the context stream, in order with
// whatever is queued there.  They touch no slot, plan, timer or diagnostic of the runs (hipcanny.hip) -- except that a reader of
// edge maps first completes the pipelined runs still writing them (finish_writers_of).  What each call does is decided in
// host_plan.h; this file checks, allocates and launches.  Product library only: the test library (libhipcanny_legacy.so) is built
// without this file and the kernel files behind it, and refuses these entries (legacy_front.hip).
// A new entry of this kind goes here: view_end (host_plan.h) gives the byte range of a view, ensure_scratch its scratch.
#include "hc_context.h"
#include "auto_thr.h"

using namespace hc;

namespace {

// At least `need` bytes in s: grows, never shrinks.  What is queued on the context stream may still read a buffer that is to be
// replaced, so that stream is waited for first; a first allocation waits for nothing (it may synchronise the device by itself)
int ensure_scratch(hc_ctx *c, DeviceScratch &s, size_t need)
{
  if (s.bytes >= need) return HC_OK;
  HIPCK(hipSetDevice(c->device));
  if (s.p) HIPCK(hipStreamSynchronize(c->stream));
  (void)hipFree(s.p);
  s = DeviceScratch{};
  HIPCK(hipMalloc(&s.p, need));
  s.bytes = need;
  return HC_OK;
}

// k_hist256 on the context stream behind the zeroing of d_hist (the view has been checked)
int queue_histogram(hc_ctx *c, const void *d_in, size_t in_pitch, size_t in_fs, int n, u32 *d_hist)
{
  HistParams hp = plan_histogram(c->W, c->H, c->C, View{ (uintptr_t)d_in, in_pitch, in_fs }, n);
  hp.hist = d_hist;
  HIPCK(hipMemsetAsync(d_hist, 0, sizeof(u32) * 256 * (size_t)n, c->stream));
  HIPCK(launch_hist256(hp, c->stream));
  return HC_OK;
}

// Pipelined runs still in flight that write into the n frames of view v (rows of row_bytes): each is completed, oldest first,
// before the view is read or written -- its hysteresis runs on another stream than the caller, and should its queued launches not
// have reached the fixpoint, its host-side continuation (finish_slot) rewrites whole maps.  As finish_overlapping, for a reader;
// the caller's buffer a staged run copies its maps to counts as well.  Runs that write elsewhere stay in flight.  A byte range
// that wraps the address space (view_end; no valid view) counts as written by every run.
int finish_writers_of(hc_ctx *c, const View &v, size_t row_bytes, int n)
{
  uintptr_t m1 = 0;
  const bool anywhere = !view_end(v, row_bytes, c->H, n, &m1);
  for (int k = 0; k < c->nslot_use; ++k) {
    Slot &o = c->slot[(c->cur + k) % c->nslot_use];
    if (!o.pending || o.stream == c->stream) continue;  // (a plain run is ordered before the reader by the context stream)
    bool hit = anywhere || (o.out0 < m1 && v.p < o.out1);
    if (!hit && o.copy_dst && o.n > 0) {
      uintptr_t d1 = 0;
      hit = !view_end(View{ (uintptr_t)o.copy_dst, o.copy_pitch, o.copy_fs }, (size_t)c->W, c->H, o.n, &d1) || ((uintptr_t)o.copy_dst < m1 && v.p < d1);
    }
    if (hit)
      if (int rc = finish_slot(c, o)) return rc;
  }
  return HC_OK;
}

// The tables [3][numangle] of hc_hough_lines_device on the device, made from `key` (hough_tables, host_plan.h).  What is queued on
// the context stream may still read the old ones, whether or not the new ones fit their allocation.
int upload_hough_tables(hc_ctx *c, const HoughTabKey &key)
{
  const size_t na = (size_t)key.numangle;
  std::vector<float> tab(3 * na);
  int a2 = 0, r2 = 0;
  if (hough_tables(c->W, c->H, key.rho, key.theta, key.min_theta, key.max_theta, &a2, &r2, tab.data(), tab.data() + na, tab.data() + 2 * na, na) || a2 != key.numangle)
    return fail(HC_E_STATE, "hc_hough_lines_device: the tables disagree with the plan");
  HIPCK(hipStreamSynchronize(c->stream));
  c->hough_key = HoughTabKey{};  // (nothing valid on the device until the copy is complete)
  if (int rc = ensure_scratch(c, c->hough_tab, sizeof(float) * 3 * na)) return rc;
  HIPCK(hipMemcpy(c->hough_tab.p, tab.data(), sizeof(float) * 3 * na, hipMemcpyHostToDevice));  // (complete when it returns)
  c->hough_key = key;
  return HC_OK;
}

// The tables [4][numangle] of hc_hough_segments_device (theta, major, slope, scale) on the device, made from `key`
// (hough_walk_tables, host_plan.h): as upload_hough_tables
int upload_seg_tables(hc_ctx *c, const HoughTabKey &key)
{
  const size_t na = (size_t)key.numangle;
  std::vector<float> ftab(3 * na);  // theta, slope, scale
  std::vector<int32_t> major(na);
  int a2 = 0;
  if (hough_walk_tables(c->W, c->H, key.rho, key.theta, key.min_theta, key.max_theta, &a2, major.data(), ftab.data() + na, ftab.data() + 2 * na, na, ftab.data())
      || a2 != key.numangle)
    return fail(HC_E_STATE, "hc_hough_segments_device: the tables disagree with the plan");
  HIPCK(hipStreamSynchronize(c->stream));
  c->seg_key = HoughTabKey{};  // (nothing valid on the device until the copies are complete)
  if (int rc = ensure_scratch(c, c->seg_tab, 16 * na)) return rc;
  char *d = (char *)c->seg_tab.p;  // the order of seg_on_scratch (host_plan.h).  Each copy is complete when it returns
  HIPCK(hipMemcpy(d, ftab.data(), 4 * na, hipMemcpyHostToDevice));
  HIPCK(hipMemcpy(d + 4 * na, major.data(), 4 * na, hipMemcpyHostToDevice));
  HIPCK(hipMemcpy(d + 8 * na, ftab.data() + na, 8 * na, hipMemcpyHostToDevice));
  c->seg_key = key;
  return HC_OK;
}

}  // namespace

extern "C" {

// Not a run (as hc_derivatives_device): the zeroing and one kernel on the context stream.
int hc_histogram_device(hc_ctx *c, const void *d_in, size_t in_pitch, size_t in_fs, int n, void *d_hist)
{
  if (!c || !d_in || !d_hist) return fail(HC_E_ARG, "hc_histogram_device: null argument");
  if ((uintptr_t)d_hist & 3u) return fail(HC_E_ARG, "hc_histogram_device: d_hist must be 4-byte aligned");
  if (int rc = check_views(c, "hc_histogram_device", n, c->max_batch, { hist_view(c, d_in, in_pitch, in_fs) })) return rc;
  HIPCK(hipSetDevice(c->device));
  return queue_histogram(c, d_in, in_pitch, in_fs, n, (u32 *)d_hist);
}

// k_hist256 into the context's scratch table, then k_auto_thr: both on the context stream, so a table the following runs
// read through hc_frame_thresholds_device needs no synchronisation.  Not a run either.  Successive calls share the scratch
// table and are ordered by the stream they are queued on (hc_set_stream between two of them: include/hipcanny.h).
int hc_auto_thresholds_device(hc_ctx *c, const void *d_in, size_t in_pitch, size_t in_fs, int n, int rule, double param, void *d_thr)
{
  if (!c || !d_in || !d_thr) return fail(HC_E_ARG, "hc_auto_thresholds_device: null argument");
  if ((uintptr_t)d_thr & 3u) return fail(HC_E_ARG, "hc_auto_thresholds_device: d_thr must be 4-byte aligned");
  if (rule != HC_AUTO_MEDIAN && rule != HC_AUTO_OTSU) return fail(HC_E_ARG, "hc_auto_thresholds_device: rule must be HC_AUTO_MEDIAN or HC_AUTO_OTSU");
  if (!auto_param_ok(rule, param)) return fail(HC_E_ARG, "hc_auto_thresholds_device: param (sigma / ratio) must lie in [0, 1]");
  if ((long long)c->W * c->H * c->C > AUTO_MAX_SAMPLES) return fail(HC_E_ARG, "hc_auto_thresholds_device: more than 2^27 samples per frame");
  if (int rc = check_views(c, "hc_auto_thresholds_device", n, c->max_batch, { hist_view(c, d_in, in_pitch, in_fs) })) return rc;
  HIPCK(hipSetDevice(c->device));
  // every refusal lies above: the table is allocated (once; the first call may synchronise the device) only by a call that runs
  if (int rc = ensure_scratch(c, c->hist256, sizeof(u32) * 256 * (size_t)c->max_batch)) return rc;
  if (int rc = queue_histogram(c, d_in, in_pitch, in_fs, n, (u32 *)c->hist256.p)) return rc;
  HIPCK(launch_auto_thr((const u32 *)c->hist256.p, n, rule, param, (int32_t *)d_thr, c->stream));
  return HC_OK;
}

// k_edge_count, k_edge_scan, k_edge_emit on the context stream (edge_points.hip).  Not a run, as hc_histogram_device -- except
// that a pipelined run in flight whose output the map overlaps is completed first (finish_writers_of).  Successive calls share
// the table of per-item counts and are ordered by the stream they are queued on (include/hipcanny.h).
int hc_edge_points_device(hc_ctx *c, const void *d_map, size_t pitch, size_t fs, int n, void *d_counts, void *d_points, size_t capacity)
{
  if (!c || !d_map || !d_counts) return fail(HC_E_ARG, "hc_edge_points_device: null argument");
  if (capacity && !d_points) return fail(HC_E_ARG, "hc_edge_points_device: d_points is null with capacity > 0");
  if ((uintptr_t)d_counts & 3u) return fail(HC_E_ARG, "hc_edge_points_device: d_counts must be 4-byte aligned");
  if ((uintptr_t)d_points & 7u) return fail(HC_E_ARG, "hc_edge_points_device: d_points must be 8-byte aligned");
  if (int rc = check_views(c, "hc_edge_points_device", n, c->max_batch * (c->per_channel ? 3 : 1), { { "d_map (pitch, fs)", d_map, pitch, fs, (size_t)c->W, 1, true } })) return rc;  // (n: at most the output frames of a max_batch run)
  const View map{ (uintptr_t)d_map, pitch, fs };
  EdgePlan P = plan_edge_points(c->W, c->H, c->C, c->max_batch, map, n, (uintptr_t)d_counts, (uintptr_t)d_points, capacity);
  if (P.error) return fail(HC_E_ARG, std::string("hc_edge_points_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  if (int rc = finish_writers_of(c, map, (size_t)c->W, n)) return rc;
  // every refusal lies above: the table is allocated (once; the first call may synchronise the device) only by a call that runs
  if (int rc = ensure_scratch(c, c->edge_items, sizeof(u32) * P.table_items)) return rc;
  P.ep.items = (u32 *)c->edge_items.p;
  HIPCK(launch_edge_points(P.ep, c->stream));
  return HC_OK;
}

// k_gauss8 on the context stream (blur.hip).  Not a run, as hc_derivatives_device -- except that a pipelined run in flight whose
// output overlaps either view is completed first (finish_writers_of, as hc_edge_points_device): a run's output is a natural
// neighbour of both views, and its hysteresis runs on another stream.
int hc_gaussian_blur_device(hc_ctx *c, const void *d_in, size_t in_pitch, size_t in_fs, void *d_out, size_t out_pitch, size_t out_fs, int n,
                            int ksize, const uint16_t *taps, int border)
{
  if (!c || !d_in || !d_out || !taps) return fail(HC_E_ARG, "hc_gaussian_blur_device: null argument");
  const size_t row = (size_t)c->C * c->W;
  if (int rc = check_views(c, "hc_gaussian_blur_device", n, c->max_batch, { { "d_in (in_pitch, in_fs)", d_in, in_pitch, in_fs, row, 1, true }, { "d_out (out_pitch, out_fs)", d_out, out_pitch, out_fs, row, 1, true } })) return rc;
  const View in{ (uintptr_t)d_in, in_pitch, in_fs }, out{ (uintptr_t)d_out, out_pitch, out_fs };
  const BlurPlan P = plan_gaussian_blur(c->W, c->H, c->C, in, out, n, ksize, taps, border);
  if (P.error) return fail(HC_E_ARG, std::string("hc_gaussian_blur_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  if (int rc = finish_writers_of(c, in, row, n)) return rc;
  if (int rc = finish_writers_of(c, out, row, n)) return rc;
  HIPCK(launch_gauss8(P.bp, c->stream));
  return HC_OK;
}

// k_hough_vote, k_hough_peaks, k_hough_scan, k_hough_rank on the context stream (hough.hip), pass after pass.  Not a run, as
// hc_histogram_device; no run writes a point list, so nothing is completed first.  Successive calls share the scratch and the
// tables and are ordered by the stream they are queued on (include/hipcanny.h).
int hc_hough_lines_device(hc_ctx *c, const void *d_points, const void *d_point_counts, size_t point_capacity, int n, double rho, double theta,
                          int threshold, double min_theta, double max_theta, void *d_line_counts, void *d_lines, size_t line_capacity)
{
  if (!c) return fail(HC_E_ARG, "hc_hough_lines_device: null argument");
  const HoughPlan P = plan_hough_lines(c->W, c->H, c->max_batch * (c->per_channel ? 3 : 1), (uintptr_t)d_points, (uintptr_t)d_point_counts, point_capacity, n, rho,
                                       theta, threshold, min_theta, max_theta, (uintptr_t)d_line_counts, (uintptr_t)d_lines, line_capacity, c->hough_bound, c->hough_rows);
  if (P.error) return fail(HC_E_ARG, std::string("hc_hough_lines_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  // every refusal lies above.  New tables or a larger scratch: what is queued on the context stream may still read the old ones
  const HoughTabKey key{ P.hp.numangle, rho, theta, min_theta, max_theta };
  if (!(c->hough_key == key))
    if (int rc = upload_hough_tables(c, key)) return rc;
  if (int rc = ensure_scratch(c, c->hough, P.scratch_bytes)) return rc;
  for (int k = 0; k < P.passes; ++k) HIPCK(launch_hough(hough_pass(P, k, (uintptr_t)c->hough.p, (uintptr_t)c->hough_tab.p), c->stream));
  return HC_OK;
}

// k_seg_count, k_seg_scan, k_seg_emit on the context stream (hough_segments.hip).  Not a run, as hc_edge_points_device, and like
// it a reader of edge maps: a pipelined run in flight whose output the map overlaps is completed first (finish_writers_of).
// Successive calls share the per-line counts and the walk tables and are ordered by the stream they are queued on.
int hc_hough_segments_device(hc_ctx *c, const void *d_map, size_t pitch, size_t fs, const void *d_lines, const void *d_line_counts, size_t line_capacity, int n,
                             double rho, double theta, double min_theta, double max_theta, int min_length, int max_gap, void *d_seg_counts, void *d_segs,
                             size_t seg_capacity)
{
  if (!c || !d_map) return fail(HC_E_ARG, "hc_hough_segments_device: null argument");
  const int max_frames = c->max_batch * (c->per_channel ? 3 : 1);  // (as hc_edge_points_device: the output frames of a max_batch run)
  if (int rc = check_views(c, "hc_hough_segments_device", n, max_frames, { { "d_map (pitch, fs)", d_map, pitch, fs, (size_t)c->W, 1, true } })) return rc;
  const View map{ (uintptr_t)d_map, pitch, fs };
  const SegPlan P = plan_hough_segments(c->W, c->H, max_frames, map, (uintptr_t)d_lines, (uintptr_t)d_line_counts, line_capacity, n, rho, theta, min_theta, max_theta,
                                        min_length, max_gap, (uintptr_t)d_seg_counts, (uintptr_t)d_segs, seg_capacity);
  if (P.error) return fail(HC_E_ARG, std::string("hc_hough_segments_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  if (int rc = finish_writers_of(c, map, (size_t)c->W, n)) return rc;
  // every refusal lies above.  New tables or a larger table of counts: what is queued on the context stream may still read the old ones
  const HoughTabKey key{ P.sp.numangle, rho, theta, min_theta, max_theta };
  if (!(c->seg_key == key))
    if (int rc = upload_seg_tables(c, key)) return rc;
  if (int rc = ensure_scratch(c, c->seg_items, P.items_bytes)) return rc;
  HIPCK(launch_hough_segments(seg_on_scratch(P, (uintptr_t)c->seg_items.p, (uintptr_t)c->seg_tab.p), c->stream));
  return HC_OK;
}

// The zeroing of the accumulators, then k_circle_vote, the peaks of hough.hip, k_circle_rank, k_circle_sift, k_circle_radii and
// k_circle_scan on the context stream (hough_circles.hip), pass after pass.  Not a run, as hc_hough_lines_device; no run writes a
// point list or a gradient plane, so nothing is completed first.  Successive calls share the scratch and are ordered by the stream
// they are queued on (include/hipcanny.h).
int hc_hough_circles_device(hc_ctx *c, const void *d_points, const void *d_point_counts, size_t point_capacity, const void *d_dx, const void *d_dy, size_t pitch,
                            size_t fs, int n, double dp, double min_dist, int votes_threshold, int min_radius, int max_radius, size_t centre_capacity,
                            void *d_circle_counts, void *d_circles, size_t circle_capacity)
{
  if (!c) return fail(HC_E_ARG, "hc_hough_circles_device: null argument");
  const CirclePlan P = plan_hough_circles(c->W, c->H, c->max_batch * (c->per_channel ? 3 : 1), (uintptr_t)d_points, (uintptr_t)d_point_counts, point_capacity,
                                          View{ (uintptr_t)d_dx, pitch, fs }, (uintptr_t)d_dy, n, dp, min_dist, votes_threshold, min_radius, max_radius, centre_capacity,
                                          (uintptr_t)d_circle_counts, (uintptr_t)d_circles, circle_capacity, c->hough_bound);
  if (P.error) return fail(HC_E_ARG, std::string("hc_hough_circles_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  // every refusal lies above.  A larger scratch: what is queued on the context stream may still read the old one
  if (int rc = ensure_scratch(c, c->circles, P.scratch_bytes)) return rc;
  for (int k = 0; k < P.passes; ++k) {
    const CircleParams cp = circle_pass(P, k, (uintptr_t)c->circles.p);
    HIPCK(hipMemsetAsync(cp.accum, 0, (size_t)cp.nframes * P.frame_accum_bytes, c->stream));
    HIPCK(launch_hough_circles(cp, c->stream));
  }
  return HC_OK;
}

// The kernels of ccl.hip on the context stream, pass after pass.  Not a run, as hc_edge_points_device; like hc_gaussian_blur_device
// it completes first a pipelined run in flight whose output overlaps either view: the map it reads or the label plane it writes.
// Successive calls share the table of per-chunk counts and are ordered by the stream they are queued on (include/hipcanny.h).
int hc_connected_components_device(hc_ctx *c, const void *d_map, size_t pitch, size_t fs, int n, int connectivity, void *d_labels, size_t label_pitch,
                                   size_t label_fs, void *d_counts, void *d_stats, void *d_centroids, size_t capacity)
{
  if (!c || !d_map || !d_labels || !d_counts) return fail(HC_E_ARG, "hc_connected_components_device: null argument");
  const int max_frames = c->max_batch * (c->per_channel ? 3 : 1);  // (as hc_edge_points_device: the output frames of a max_batch run)
  const size_t row = (size_t)c->W, label_row = 4 * (size_t)c->W;
  if (int rc = check_views(c, "hc_connected_components_device", n, max_frames, { { "d_map (pitch, frame_stride)", d_map, pitch, fs, row, 1, true }, { "d_labels (label_pitch, label_frame_stride)", d_labels, label_pitch, label_fs, label_row, 4, true } })) return rc;
  const View map{ (uintptr_t)d_map, pitch, fs }, labels{ (uintptr_t)d_labels, label_pitch, label_fs };
  const CclPlan P = plan_connected_components(c->W, c->H, max_frames, map, labels, n, connectivity, (uintptr_t)d_counts, (uintptr_t)d_stats, (uintptr_t)d_centroids,
                                              capacity, c->hough_bound);
  if (P.error) return fail(HC_E_ARG, std::string("hc_connected_components_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  if (int rc = finish_writers_of(c, map, row, n)) return rc;
  if (int rc = finish_writers_of(c, labels, label_row, n)) return rc;
  // every refusal lies above.  A larger table: what is queued on the context stream may still read the old one
  if (int rc = ensure_scratch(c, c->ccl_items, P.scratch_bytes)) return rc;
  for (int k = 0; k < P.passes; ++k) HIPCK(launch_connected_components(ccl_pass(P, k, (uintptr_t)c->ccl_items.p), c->stream));
  return HC_OK;
}

// One or two launches of k_morph8 per pass on the context stream (morph.hip).  Not a run, as hc_gaussian_blur_device, and like it
// it completes first a pipelined run in flight whose output overlaps either view.  `channels` is the caller's: edge maps have one
// channel on every context.  OPEN and CLOSE keep their intermediate frames in the context's scratch; successive calls share it and
// are ordered by the stream they are queued on (include/hipcanny.h).
int hc_morphology_device(hc_ctx *c, const void *d_in, size_t in_pitch, size_t in_fs, void *d_out, size_t out_pitch, size_t out_fs, int n, int channels, int op,
                         int ksize, const int8_t *spans)
{
  if (!c || !d_in || !d_out || !spans) return fail(HC_E_ARG, "hc_morphology_device: null argument");
  const View in{ (uintptr_t)d_in, in_pitch, in_fs }, out{ (uintptr_t)d_out, out_pitch, out_fs };
  const MorphPlan P = plan_morphology(c->W, c->H, c->C, c->per_channel != 0, c->max_batch, in, out, n, channels, op, ksize, spans, c->hough_bound);
  if (P.error) return fail(HC_E_ARG, std::string("hc_morphology_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  const size_t row = (size_t)channels * c->W;
  if (int rc = finish_writers_of(c, in, row, n)) return rc;
  if (int rc = finish_writers_of(c, out, row, n)) return rc;
  // every refusal lies above.  A larger scratch: what is queued on the context stream may still read the old one
  if (P.scratch_bytes)
    if (int rc = ensure_scratch(c, c->morph_mid, P.scratch_bytes)) return rc;
  for (int k = 0; k < P.passes; ++k) {
    const MorphPass mp = morph_pass(P, k, (uintptr_t)c->morph_mid.p);
    for (int s = 0; s < mp.stages; ++s) HIPCK(launch_morph8(mp.st[s], c->stream));
  }
  return HC_OK;
}

// k_dt_cols, then k_dt_rows on the context stream (dist.hip).  Not a run, as hc_connected_components_device, and like it it
// completes first a pipelined run in flight whose output overlaps any of its views: the map it reads, the distance plane or the
// nearest plane it writes.  No scratch: the dy of the column pass live in the caller's distance plane between the two kernels.
int hc_distance_transform_device(hc_ctx *c, const void *d_map, size_t pitch, size_t fs, int n, int target, int dist_type, void *d_dist, size_t dist_pitch,
                                 size_t dist_fs, void *d_nearest, size_t nearest_pitch, size_t nearest_fs)
{
  if (!c || !d_map || !d_dist) return fail(HC_E_ARG, "hc_distance_transform_device: null argument");
  const int max_frames = c->max_batch * (c->per_channel ? 3 : 1);  // (as hc_edge_points_device: the output frames of a max_batch run)
  const size_t row = (size_t)c->W, word_row = 4 * (size_t)c->W;
  const View map{ (uintptr_t)d_map, pitch, fs }, dist{ (uintptr_t)d_dist, dist_pitch, dist_fs };
  const View nearest = d_nearest ? View{ (uintptr_t)d_nearest, nearest_pitch, nearest_fs } : View{ 0, 0, 0 };
  if (int rc = check_views(c, "hc_distance_transform_device", n, max_frames, { { "d_map (pitch, frame_stride)", d_map, pitch, fs, row, 1, true }, { "d_dist (dist_pitch, dist_frame_stride)", d_dist, dist_pitch, dist_fs, word_row, 4, true } })) return rc;
  if (d_nearest)
    if (int rc = check_views(c, "hc_distance_transform_device", n, max_frames, { { "d_nearest (nearest_pitch, nearest_frame_stride)", d_nearest, nearest_pitch, nearest_fs, word_row, 4, true } })) return rc;
  const DistPlan P = plan_distance_transform(c->W, c->H, max_frames, map, dist, nearest, n, target, dist_type);
  if (P.error) return fail(HC_E_ARG, std::string("hc_distance_transform_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  if (int rc = finish_writers_of(c, map, row, n)) return rc;
  if (int rc = finish_writers_of(c, dist, word_row, n)) return rc;
  if (d_nearest)
    if (int rc = finish_writers_of(c, nearest, word_row, n)) return rc;
  // every refusal lies above
  HIPCK(launch_distance_transform(P.dp, c->stream));
  return HC_OK;
}

// Per pass the zeroing of the removal tables, k_thin_pack, 2 * max_iterations launches of k_thin_step and k_thin_unpack on the
// context stream (thin.hip).  Not a run, as hc_morphology_device, and like it it completes first a pipelined run in flight whose
// output overlaps either view.  The bit planes and the tables live in the context's scratch; successive calls share it and are
// ordered by the stream they are queued on (include/hipcanny.h).
int hc_thinning_device(hc_ctx *c, const void *d_map, size_t pitch, size_t fs, void *d_out, size_t out_pitch, size_t out_fs, int n, int method, int max_iterations,
                       void *d_status)
{
  if (!c || !d_map || !d_out) return fail(HC_E_ARG, "hc_thinning_device: null argument");
  const View map{ (uintptr_t)d_map, pitch, fs }, out{ (uintptr_t)d_out, out_pitch, out_fs };
  const ThinPlan P = plan_thinning(c->W, c->H, c->per_channel != 0, c->max_batch, map, out, n, method, max_iterations, (uintptr_t)d_status, c->hough_bound);
  if (P.error) return fail(HC_E_ARG, std::string("hc_thinning_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  const size_t row = (size_t)c->W;
  if (int rc = finish_writers_of(c, map, row, n)) return rc;
  if (int rc = finish_writers_of(c, out, row, n)) return rc;
  // every refusal lies above.  A larger scratch: what is queued on the context stream may still read the old one
  if (int rc = ensure_scratch(c, c->thin, P.scratch_bytes)) return rc;
  for (int k = 0; k < P.passes; ++k) {
    const ThinPass tp = thin_pass(P, k, (uintptr_t)c->thin.p);
    HIPCK(hipMemsetAsync((void *)tp.tables, 0, tp.tables_bytes, c->stream));
    HIPCK(launch_thin_pack(tp.pack, c->stream));
    for (int it = 1; it <= P.max_iterations; ++it)
      for (int s = 0; s < 2; ++s) HIPCK(launch_thin_step(tp.step, s, it, c->stream));
    HIPCK(launch_thin_unpack(tp.unpack, c->stream));
  }
  return HC_OK;
}

// One launch of k_corner_response on the context stream (corners.hip).  Not a run, exactly as hc_derivatives_device is none, whose
// planes it reads: no run writes an int16 or a float32 plane, so nothing is completed first.  No scratch.
int hc_corner_response_device(hc_ctx *c, const void *d_dx, const void *d_dy, size_t pitch, size_t fs, void *d_response, size_t out_pitch, size_t out_fs, int n,
                              int block_size, int method, double harris_k)
{
  if (!c) return fail(HC_E_ARG, "hc_corner_response_device: null argument");
  const CornerPlan P = plan_corner_response(c->W, c->H, c->max_batch * (c->per_channel ? 3 : 1), View{ (uintptr_t)d_dx, pitch, fs }, (uintptr_t)d_dy,
                                            View{ (uintptr_t)d_response, out_pitch, out_fs }, n, block_size, method, harris_k);
  if (P.error) return fail(HC_E_ARG, std::string("hc_corner_response_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  // every refusal lies above
  HIPCK(launch_corner_response(P.cp, c->stream));
  return HC_OK;
}

// Per pass the zeroing of the histograms and state words and the kernels of launch_good_features on the context stream
// (corners.hip).  Not a run, as hc_hough_circles_device; no run writes a float32 plane, so nothing is completed first.  Successive
// calls share the scratch and are ordered by the stream they are queued on (include/hipcanny.h).
int hc_good_features_device(hc_ctx *c, const void *d_response, size_t pitch, size_t fs, int n, double quality_level, double min_distance, size_t candidate_capacity,
                            void *d_corner_counts, void *d_corners, void *d_quality, size_t corner_capacity)
{
  if (!c) return fail(HC_E_ARG, "hc_good_features_device: null argument");
  const FeatPlan P = plan_good_features(c->W, c->H, c->max_batch * (c->per_channel ? 3 : 1), View{ (uintptr_t)d_response, pitch, fs }, n, quality_level, min_distance,
                                        candidate_capacity, (uintptr_t)d_corner_counts, (uintptr_t)d_corners, (uintptr_t)d_quality, corner_capacity, c->hough_bound);
  if (P.error) return fail(HC_E_ARG, std::string("hc_good_features_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  // every refusal lies above.  A larger scratch: what is queued on the context stream may still read the old one
  if (int rc = ensure_scratch(c, c->feat, P.scratch_bytes)) return rc;
  for (int k = 0; k < P.passes; ++k) {
    const FeatPass fp = feat_pass(P, k, (uintptr_t)c->feat.p);
    HIPCK(hipMemsetAsync((void *)fp.zero, 0, fp.zero_bytes, c->stream));
    HIPCK(launch_good_features(fp.fp, c->stream));
  }
  return HC_OK;
}

// One launch of k_pyr_down8 on the context stream (flow.hip).  Not a run, as hc_morphology_device, and like it it completes first a
// pipelined run in flight whose output overlaps either view: u8 planes may be run outputs.  No scratch.
int hc_pyr_down_device(hc_ctx *c, const void *d_src, size_t pitch, size_t fs, int src_width, int src_height, void *d_dst, size_t dst_pitch, size_t dst_fs, int n)
{
  if (!c) return fail(HC_E_ARG, "hc_pyr_down_device: null argument");
  const View src{ (uintptr_t)d_src, pitch, fs }, dst{ (uintptr_t)d_dst, dst_pitch, dst_fs };
  const PyrPlan P = plan_pyr_down(c->W, c->H, c->max_batch * (c->per_channel ? 3 : 1), src, src_width, src_height, dst, n);
  if (P.error) return fail(HC_E_ARG, std::string("hc_pyr_down_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  // (finish_writers_of takes the context's height for the views' byte ranges: a level is no taller)
  if (int rc = finish_writers_of(c, src, (size_t)src_width, n)) return rc;
  if (int rc = finish_writers_of(c, dst, (size_t)P.pp.dW, n)) return rc;
  // every refusal lies above
  HIPCK(launch_pyr_down(P.pp, c->stream));
  return HC_OK;
}

// One launch of k_lk_flow on the context stream (flow.hip): one pyramid level of the tracker.  Not a run; like hc_pyr_down_device it
// completes first a pipelined run in flight whose output overlaps either image.  No scratch.
int hc_lk_flow_device(hc_ctx *c, const void *d_prev, const void *d_next, size_t pitch, size_t fs, int width, int height, int level, int n, const void *d_counts,
                      const void *d_prev_pts, void *d_next_pts, size_t capacity, int win, int max_iterations, double epsilon, double min_eig_threshold, int use_initial,
                      void *d_status, void *d_err)
{
  if (!c) return fail(HC_E_ARG, "hc_lk_flow_device: null argument");
  const View prev{ (uintptr_t)d_prev, pitch, fs }, next{ (uintptr_t)d_next, pitch, fs };
  const FlowPlan P = plan_lk_flow(c->W, c->H, c->max_batch * (c->per_channel ? 3 : 1), prev, (uintptr_t)d_next, width, height, level, n, (uintptr_t)d_counts,
                                  (uintptr_t)d_prev_pts, (uintptr_t)d_next_pts, capacity, win, max_iterations, epsilon, min_eig_threshold, use_initial, (uintptr_t)d_status,
                                  (uintptr_t)d_err);
  if (P.error) return fail(HC_E_ARG, std::string("hc_lk_flow_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  if (int rc = finish_writers_of(c, prev, (size_t)width, n)) return rc;
  if (int rc = finish_writers_of(c, next, (size_t)width, n)) return rc;
  // every refusal lies above
  HIPCK(launch_lk_flow(P.fp, c->stream));
  return HC_OK;
}

}  // extern "C"
