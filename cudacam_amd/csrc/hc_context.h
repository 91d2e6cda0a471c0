// hc_context.h -- the context behind the C ABI (include/hipcanny.h) and what every host file of the library shares: the slots
// and the profiling ring of the runs, the error text, the view checks of the entry points.  Internal, host only.
// hipcanny.hip owns the runs; device_ops.hip holds the entries that are not runs (product library only).
#pragma once
#include "../../include/hipcanny.h"
#include "canny_common.h"
#include "host_plan.h"

#include <initializer_list>
#include <string>
#include <vector>

namespace hc {

extern thread_local std::string g_err;  // hc_last_error's text: one object for the library, defined in hipcanny.hip
inline int fail(int code, const std::string &msg)
{
  g_err = msg;
  return code;
}
#define HIPCK(expr)                                                                                   \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return fail(HC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));  \
  } while (0)

// Everything one in-flight fused run owns (how many slots a context uses: pipeline_slots, host_plan.h); the plain mode
// only uses slot 0.
struct Slot {
  bool complete = false;                       // every allocation below succeeded (alloc_slot)
  u32 *d_sbits = nullptr, *d_cbits = nullptr;  // bit planes [max_batch][H][RD]
  u32 *d_wl_list = nullptr;  // hysteresis worklists (HystParams::wl_list)
  size_t wl_cap = 0;         // tiles a run can have
  u32 *d_flags = nullptr, *h_flags = nullptr;
  hipEvent_t ev_front = nullptr, ev_done = nullptr;  // front kernel finished / hysteresis + expand finished
  bool pending = false;                              // convergence flag not yet checked by the host
  HystParams ph{};  // parameters of this run's hysteresis launches (lists, late_grid, iter, stats: set per launch from `plan`)
  HystPlan plan;    // its schedule: what was queued, what a continuation repeats, what hc_last_hysteresis_schedule reports
  void *copy_dst = nullptr;  // caller buffer when the expand went to the internal one
  size_t copy_pitch = 0, copy_fs = 0;
  int n = 0;
  bool prov = false;             // this run's k_nms wrote the provisional output
  hipStream_t stream = nullptr;  // stream the hysteresis of this run was queued on
  hipStream_t s_hyst = nullptr;  // this slot's hysteresis stream (pipelined mode)
  uintptr_t out0 = 0, out1 = 0;  // output range of this (pipelined, still pending) run: a later run into the same memory waits for it
  unsigned long long seq = 0;    // number of the pipelined run that uses the slot (hc_ctx::run_seq)
};

// hipEvent ring of the profiled runs: up to EV_PER_RUN events per run.  Interval i = ev[i] -> ev[i + 1] covers the reference
// stages in RunProf::mask[i] (one kernel may cover several: its time is divided equally among them, see hc_stage_time_ms)
struct ProfRing {
  static constexpr int EV_RUNS = 256;
  static constexpr int EV_PER_RUN = 8;
  enum { K_STAGE0 = 0, K_FRONT_A = 1, K_FRONT_B = 2, K_HYST = 3 };  // grey kernel / k_blur / k_nms, the fused front kernel or the tap kernels / hysteresis
  struct RunProf { int nint = 0; bool after_gap = false; uint8_t mask[EV_PER_RUN - 1] = { 0 }; uint8_t kind[EV_PER_RUN - 1] = { 0 }; };
  bool on = false;
  bool gap = false;  // a run went untimed since the last timed one (ring full)
  std::vector<hipEvent_t> evpool;
  std::vector<RunProf> runprof;
  int head = 0, count = 0;    // runs recorded since the last collect
  hipEvent_t *ev = nullptr;   // the events of the run being queued (null: it goes untimed)
  RunProf *rp = nullptr;
  float stage_ms[6] = { 0, 0, 0, 0, 0, 0 };
  unsigned stage_ran = 0;         // stages the last profiled run executed (bit per stage)
  double sum[3] = { 0, 0, 0 };
  double split_sum[2] = { 0, 0 };  // k_blur, k_nms (split front path only)
  long split_runs = 0;
  long runs = 0;
  std::vector<float> step_ms;     // end-of-run to end-of-run intervals of consecutive profiled runs (steady-state step time)
  std::vector<float> front_each;  // the front kernels' time of every profiled HYSTER run (hc_profile_get_front_each)
  hipEvent_t prev_end = nullptr;  // last event of the previous profiled run (its ring slot is not reused before the next collect: at most EV_RUNS - 1 runs are in flight)

  hipError_t begin_run(hipStream_t st)
  {
    ev = nullptr; rp = nullptr;
    // ring full: this run goes untimed.  One slot stays free: `prev_end` still points at the last event of the run collected
    // last, and a 256th queued run would record over it
    if (!on || count >= EV_RUNS - 1) {
      if (on) gap = true;  // the next timed run's step interval would span this one
      return hipSuccess;
    }
    const size_t slot_i = (size_t)((head + count) % EV_RUNS);
    ev = &evpool[slot_i * EV_PER_RUN];
    rp = &runprof[slot_i];
    *rp = RunProf{};
    rp->after_gap = gap;
    gap = false;
    return hipEventRecord(ev[0], st);
  }
  // closes the interval that began at the previous event: it covered `mask` (bit per reference stage)
  hipError_t mark(hipStream_t st, unsigned mask, int kind)
  {
    if (!rp || rp->nint >= EV_PER_RUN - 1) return hipSuccess;
    rp->mask[rp->nint] = (uint8_t)mask;
    rp->kind[rp->nint] = (uint8_t)kind;
    rp->nint++;
    return hipEventRecord(ev[rp->nint], st);
  }
  void end_run() { if (rp) count++; }
  // the event intervals of every run recorded since the last collect (all of them complete: hc_sync)
  int collect()
  {
    for (; count > 0; head = (head + 1) % EV_RUNS, count--) {
      hipEvent_t *e = &evpool[(size_t)head * EV_PER_RUN];
      const RunProf &r = runprof[(size_t)head];
      for (float &m : stage_ms) m = 0;
      stage_ran = 0;
      bool has_a = false, has_h = false;
      float front_t = 0;
      for (int i = 0; i < r.nint; ++i) has_a = has_a || r.kind[i] == K_FRONT_A;
      for (int i = 0; i < r.nint; ++i) has_h = has_h || r.kind[i] == K_HYST;
      for (int i = 0; i < r.nint; ++i) {
        float t = 0;
        HIPCK(hipEventElapsedTime(&t, e[i], e[i + 1]));
        if (r.kind[i] == K_FRONT_A || r.kind[i] == K_FRONT_B) front_t += t;
        const unsigned mask = r.mask[i];
        const int nst = __builtin_popcount(mask);
        for (int st = 0; st < 6; ++st)
          if (mask >> st & 1u) stage_ms[st] += t / (float)nst;
        stage_ran |= mask;
        const int k = r.kind[i];
        sum[k == K_STAGE0 ? 0 : k == K_HYST ? 2 : 1] += t;
        if (k == K_FRONT_A) split_sum[0] += t;
        else if (k == K_FRONT_B && has_a) split_sum[1] += t;
      }
      if (has_a) split_runs++;
      if (has_h && front_each.size() < 65536) front_each.push_back(front_t);
      if (r.nint > 0) {
        if (prev_end && !r.after_gap && step_ms.size() < 65536) {
          float dt = 0;
          if (hipEventElapsedTime(&dt, prev_end, e[r.nint]) == hipSuccess) step_ms.push_back(dt);
        }
        prev_end = e[r.nint];
      }
      runs++;
    }
    return HC_OK;
  }
};

// A lazily allocated device buffer that only grows (ensure_scratch, device_ops.hip)
struct DeviceScratch { void *p = nullptr; size_t bytes = 0; };
// what the Hough tables on the device were made from
struct HoughTabKey {
  int numangle = 0;
  double rho = 0, theta = 0, min_theta = 0, max_theta = 0;
  bool operator==(const HoughTabKey &o) const { return numangle == o.numangle && rho == o.rho && theta == o.theta && min_theta == o.min_theta && max_theta == o.max_theta; }
};
}  // namespace hc

struct hc_ctx {
  int device = 0, W = 0, H = 0, C = 1, max_batch = 1, mode = HC_MODE_R;
  int RD = 0, nstrips = 0;
  int per_channel = 0;  // 3-channel input: one edge map per channel (3 output frames per input frame)
  hc::FrontOpts opt;        // thresholds and the caller's choices for the front path
  hc::HystOpts hopt;        // hc_set_tuning, the HC_OPT_TEST_HYST_* hooks and (read ONCE at hc_create, never in the launch path) HC_HYST_DIAG / HC_HYST_GEOM
  hipStream_t own_stream = nullptr, stream = nullptr;  // context stream (own, or the caller's)
  // internal pitched frames
  uint8_t *d_in = nullptr, *d_mono = nullptr, *d_out = nullptr;
  size_t in_pitch = 0, in_fs = 0, mono_pitch = 0, mono_fs = 0, out_pitch = 0, out_fs = 0;
  // stage-tap scratch (lazy)
  uint8_t *d_blur = nullptr, *d_nms = nullptr;
  int16_t *d_sx = nullptr, *d_sy = nullptr;
  uint8_t *d_dump = nullptr;    // k_front8's dump areas (FrontParams::dump / dump_c / dump_p), followed by its page of zeros (FrontParams::zeros)
  size_t dump_region = 0;       // 0: the plain layout (16 KiB + 32 KiB); otherwise four regions of this size (the HALF form's lane offsets reach a frame further)
  uint8_t *d_bplane = nullptr;  // split mode: u8 blur plane between the two kernels (lazy)
  size_t bplane_fs = 0, bplane_frames = 0;
  // fused path
  hc::Slot slot[hc::NSLOT];
  int nslot_use = 2;  // slots the pipelined runs rotate through (4 for small batches)
  int cur = 0;
  bool pipeline = false;
  unsigned long long run_seq = 0;
  hc::ChainWatch watch;   // two or three slots, one-wave or four-wave front workgroups: by the timestamps below (watch_chain)
  struct { hipEvent_t f[8] = {}, d[8] = {}; unsigned long long seq[8] = {}; } ring;  // of the last pipelined runs, by run number & 7: front kernel finished / hysteresis finished
  hc::HystHistory hist;   // what the finished runs needed (plan_hyst)
  hc::ProfRing prof;
  struct {  // hc_download_begin .. hc_download_end
    uint8_t *host = nullptr; size_t row = 0, fs = 0; int n = 0;
    bool stale = false;  // a host-side hysteresis continuation rewrote maps after hc_download_begin queued their copy (whichever entry point ran it)
  } dl;
  // HC_OPT_COPY_STREAMS: uploads / downloads on the device's shared copy streams, tied to the context stream by events
  bool copy_streams = false;
  hipEvent_t ev_up = nullptr, ev_ready = nullptr, ev_ready2 = nullptr, ev_down = nullptr;
  hipEvent_t ev_switch = nullptr;  // hc_set_stream / hc_use_own_stream: the end of the outgoing stream, which the incoming one waits for (created by the first switch)
  struct {  // HC_OPT_DEBUG_TAPS: copies of the bit planes as the front kernels left them, and (fused kernel) a plain blur plane
    hc::u32 *s = nullptr, *c = nullptr;
    uint8_t *blur = nullptr;
    int frames = 0;  // output frames captured by the last run (0: nothing captured)
    bool blur_split = false, blur_valid = false;
  } dbg;
  struct {  // diagnostics of the last run(s); decide nothing
    int front_waves = 4;  // waves per workgroup of the most recent k_front8 launch
    int in_staged = 0, out_staged = 0, front_form = HC_FORM_FRONT_O;  // what the last run did with the caller's buffers / which front kernels it used
    int continued = 0;
    int sched[HC_SCHED_WORDS] = { 0 };  // hc_last_hysteresis_schedule: the schedule of the last completed run
    hc::u32 stats[3 * hc::MAX_HYST_LAUNCHES] = { 0 };
    unsigned long long totals[4] = { 0, 0, 0, 0 };  // runs, continued runs, launches with work, launches queued
    int run_n = 0;
    int slot = 0;  // slot of the most recent fused run
  } last;
  int uploaded = 0;
  // Mode O: the per-frame threshold table of the runs that follow (hc_frame_thresholds_device; caller-owned device memory,
  // read by the front kernels only) and how many frames it holds; null: the context's pair
  const int32_t *frame_thr = nullptr;
  int frame_thr_n = 0;
  // lazily allocated scratch of the device-op entries (device_ops.hip: ensure_scratch), freed by hc_destroy
  hc::DeviceScratch hist256;     // hc_auto_thresholds_device: histograms [max_batch][256] between k_hist256 and k_auto_thr
  hc::DeviceScratch edge_items;  // hc_edge_points_device: per-work-item counts / offsets between its three kernels
  // hc_hough_lines_device: the scratch of one pass [peak lists | accumulators | per-row counts], grown when a call needs more; the
  // tables [3][numangle] on the device and the arguments they were made from (width and height are the context's)
  hc::DeviceScratch hough, hough_tab;
  hc::HoughTabKey hough_key;
  size_t hough_bound = hc::HOUGH_SCRATCH_BYTES;  // (HC_OPT_TEST_HOUGH_SCRATCH)
  int hough_rows = 0;  // HC_OPT_TEST_HOUGH_ROWS: angles per workgroup of k_hough_vote; 0: by the plan's rule
  // hc_hough_segments_device: kept segments / offsets per line slot [nframes][line_capacity]; its tables [4][numangle] (theta, major,
  // slope, scale) on the device and the arguments they were made from
  hc::DeviceScratch seg_items, seg_tab;
  hc::HoughTabKey seg_key;
  // hc_hough_circles_device: the scratch of one pass [ranked centres | kept centres | peak lists | accumulators | per-row counts |
  // per-centre counts | peak and kept totals] (circle_pass, host_plan.h), bounded by hough_bound as well
  hc::DeviceScratch circles;
  // hc_connected_components_device: the roots / offsets per chunk of rows of one pass (ccl_pass, host_plan.h), bounded by hough_bound as well
  hc::DeviceScratch ccl_items;
  // hc_morphology_device: the frames between the two stages of HC_MORPH_OPEN / HC_MORPH_CLOSE of one pass (morph_pass, host_plan.h),
  // bounded by hough_bound as well
  hc::DeviceScratch morph_mid;
  // hc_thinning_device: the two bit planes and the removal table of every frame of one pass (thin_pass, host_plan.h), bounded by
  // hough_bound as well
  hc::DeviceScratch thin;
  // hc_good_features_device: the candidate, ranked and kept lists, the histogram, the state words and the per-row counts of every
  // frame of one pass (feat_pass, host_plan.h), bounded by hough_bound as well
  hc::DeviceScratch feat;
};

namespace hc {

// hipcanny.hip, for device_ops.hip: completes a queued fused run (finish_writers_of)
int finish_slot(hc_ctx *c, Slot &s);

// A caller's view as an entry point names it, and what the entry demands of it (check_view, host_plan.h)
struct ViewArg { const char *name; const void *p; size_t pitch, fs, row_bytes; unsigned align = 1; bool below_4g = false; };
// Every refusal of a pitched batch view: nframes within 1 .. max_frames, then each view -> HC_E_ARG "<entry>: <view>: <rule>"
inline int check_views(const hc_ctx *c, const char *entry, int n, int max_frames, std::initializer_list<ViewArg> views)
{
  const std::string who(entry);
  if (n <= 0 || n > max_frames) return fail(HC_E_ARG, who + ": nframes out of range");
  for (const ViewArg &a : views)
    if (const ViewFault f = check_view(View{ (uintptr_t)a.p, a.pitch, a.fs }, a.row_bytes, c->H, n, a.align, a.below_4g))
      return fail(HC_E_ARG, who + ": " + a.name + ": " + VIEW_FAULT_TEXT[f]);
  return HC_OK;
}
// the view hc_histogram_device and hc_auto_thresholds_device take: any alignment, below 4 GiB
inline ViewArg hist_view(const hc_ctx *c, const void *d_in, size_t in_pitch, size_t in_fs) { return { "d_in (in_pitch, in_fs)", d_in, in_pitch, in_fs, (size_t)c->C * c->W, 1, true }; }
// host views (hc_upload, hc_download, hc_download_begin, hc_debug_tap): the rows only, as ever -- their frames may lie anywhere
inline int check_host_rows(const char *entry, size_t row_stride, size_t row_bytes)
{
  if (const ViewFault f = check_view(View{ 0, row_stride, 0 }, row_bytes, 1, 1, 1, false)) return fail(HC_E_ARG, std::string(entry) + ": row_stride: " + VIEW_FAULT_TEXT[f]);
  return HC_OK;
}

}  // namespace hc
