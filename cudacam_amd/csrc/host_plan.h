// host_plan.h -- every scheduling decision of the library as plain functions: which front kernel form a run gets and
// how its work is cut (plan_front: stage_views, choose_form, one cut_* function per kernel family), the hysteresis launch schedule (plan_hyst) and what it learns from finished runs
// (HystHistory), the slot count of pipelined runs (pipeline_slots, ChainWatch); what every device entry point refuses of a
// caller's pitched view (check_view) and the kernel parameters of the entries that are not runs (plan_derivatives,
// plan_histogram, plan_edge_points, plan_gaussian_blur, plan_hough_lines, plan_hough_segments, plan_hough_circles, plan_connected_components, plan_morphology, plan_distance_transform, plan_thinning, plan_corner_response, plan_good_features, plan_pyr_down, plan_lk_flow; the taps rule of
// hc_gaussian_taps_q8, the table rules of hc_hough_tables and hc_hough_walk_tables and the geometry of hc_hough_circle_geometry).  No HIP, no hc_ctx: hipcanny.hip fills
// the inputs, patches the device pointers in and launches; tests/cpp/plan_driver.cpp checks the plans without a GPU.
#pragma once
#include "../../include/hipcanny.h"
#include "canny_params.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace hc {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline bool aligned4(uintptr_t p, size_t a, size_t b) { return ((p | a | b) & 3u) == 0; }
inline bool reaches_4g(int H, size_t pitch) { return pitch > 0xFFFFFFFFull / (size_t)H; }  // H * pitch >= 2^32, by a division: no pitch wraps it

// ---- caller views ---------------------------------------------------------------------------------
struct View { uintptr_t p; size_t pitch, fs; };  // a pitched batch of frames: address, bytes per row, bytes per frame
enum ViewFault { VIEW_OK = 0, VIEW_PITCH, VIEW_STRIDE, VIEW_ALIGN, VIEW_4G };
constexpr const char *VIEW_FAULT_TEXT[] = { "", "pitch smaller than a row", "frame stride below height * pitch", "address, pitch and frame stride must be multiples of the element size (int16 planes: even)", "views of 4 GiB and more (height * pitch >= 2^32) are not supported by this entry" };
// What every device entry point asks of a view (hc_context.h: check_views), the first rule broken: the pitch holds a row; n > 1: the
// frame stride holds a frame; address, pitch and frame stride are multiples of `align` (1, 2, 4); below_4g (kernels with 32-bit row
// offsets): height * pitch < 2^32.  No product is formed, so none wraps: no huge pitch slips past the stride and 4 GiB tests.
inline ViewFault check_view(const View &v, size_t row_bytes, int H, int n, unsigned align, bool below_4g)
{
  if (v.pitch < row_bytes) return VIEW_PITCH;
  if (n > 1 && v.fs / (size_t)H < v.pitch) return VIEW_STRIDE;
  if ((v.p | v.pitch | v.fs) & (align - 1)) return VIEW_ALIGN;
  return below_4g && reaches_4g(H, v.pitch) ? VIEW_4G : VIEW_OK;
}
// [v.p, *end): n frames of H rows of row_bytes.  false: the range wraps the address space (*end untouched)
// The one statement of a view's byte range, p + (n - 1) fs + (H - 1) pitch + row_bytes (H, n >= 1).  As check_view, it forms no
// product or sum before a division or subtraction has shown that it fits.
inline bool view_end(const View &v, size_t row_bytes, int H, int n, uintptr_t *end)
{
  const size_t rows = (size_t)(H - 1), steps = (size_t)(n - 1);
  if (rows && v.pitch > (UINTPTR_MAX - row_bytes) / rows) return false;
  const size_t frame = rows * v.pitch + row_bytes;
  if (steps && v.fs > (UINTPTR_MAX - frame) / steps) return false;
  const size_t bytes = steps * v.fs + frame;
  if (v.p > UINTPTR_MAX - bytes) return false;
  *end = v.p + bytes;
  return true;
}

constexpr int MAX_HYST_LAUNCHES = 96;  // (48 until a weak edge wobbling along a tile boundary needed 52: one launch per crossing)
constexpr int FLAG_WORDS = MAX_HYST_LAUNCHES * 4;  // [0 .. MAX) launch flags, then 3 diagnostic words per launch
// d_flags continues with what must also be zero when a run starts (one memset): the worklist counts of the hysteresis
// launches, then the per-tile reason words of both launch parities (HystParams::wl_count / wl_reason)
constexpr int WL_COUNT_WORDS = 128;
static_assert(WL_COUNT_WORDS >= MAX_HYST_LAUNCHES + 1 + 2, "a count per launch, one beyond the last, and the two words of k_hyst_loop's barrier");
// tiles a run can have: at most out_frames x row tiles (16 rows or more each) x column panels
inline size_t slot_wl_cap(size_t out_frames, int H, int RD) { return out_frames * ((size_t)(H + 15) / 16 + 1) * (size_t)((RD + 63) / 64); }
// words of a slot's d_flags / words of them a run of wl_stride tiles needs zero when it starts
inline size_t run_flag_words(size_t wl_stride) { return FLAG_WORDS + WL_COUNT_WORDS + 2 * wl_stride; }

// ---- what hc_create derives from the frame size -------------------------------------------------
// internal frame buffers: rows of whole 16-byte groups are stored tight, others padded to 256 bytes (alloc_frames)
inline size_t frame_pitch(size_t row_bytes, size_t tight_row_bytes) { return (tight_row_bytes && tight_row_bytes % 16 == 0) ? tight_row_bytes : round_up(row_bytes, 256); }
// bit-plane row: covers every strip's 31 bytes, padded to a multiple of 64 dwords (one LDS row per wave); 0: too wide
inline int plane_row_dwords(int W)
{
  const size_t need = std::max<size_t>((size_t)(W + 31) / 32, ((size_t)((W + STRIP_W - 1) / STRIP_W) * 31 + 3) / 4);
  return need > 256 ? 0 : need <= 64 ? 64 : need <= 128 ? 128 : 256;  // 1, 2 or 4 column panels of 64 dwords
}
// narrow frames take k_front8's HALF form when that needs fewer waves: an odd number of half-strips (pairs across frames)
inline bool half_pays(int W) { return front8_half_strips(W) % 2 == 1 || (front8_half_strips(W) + 1) / 2 < front8_strips(W); }
// size of each of the four dump regions the HALF form needs: half-wave B reaches its frame through lane offsets of up to
// one frame stride (three bit-plane / output frames in per-channel mode)
inline size_t half_dump_region(size_t in_fs, size_t out_fs, int RD, int H) { return round_up(std::max(std::max(in_fs, 3 * out_fs), 3 * sizeof(u32) * (size_t)RD * H) + 32768, 4096); }

// Slots a pipelined context rotates through.  Two slots let run i+1's front kernel overlap run i's hysteresis.  Big batches
// rotate through two -- or three, while the hysteresis chain of a run is seen to outlast the front kernel of the next
// (ChainWatch; 8K x 3: 6.9 -> 7.8 k frames/s, 8K grey 25.3 -> 27.5 k; where the front kernel bounds the step a third slot
// costs 1 %, a fourth 4 %: profiles/r03/experiments.md).  SMALL batches use four slots, each with a hysteresis stream of
// its own: there a step is the latency of the hysteresis' chain of dependent launches (8 frames: 0.33 ms for a 0.04 ms
// front kernel), and chains of different runs share the device without noticing each other.
constexpr int NSLOT = 4;
// slots the pipelined runs of n_out output frames rotate through: by pixels (16 8K x 3 frames are a big batch; fewer than
// 0.5 G pixels per run: the step is the latency of the hysteresis chain)
// (measured at 1080p: 128 frames per run 237 against 218 k frames/s with four, 256 frames 301 against 310 k)
inline int pipeline_slots(int pipe_slots, int big_slots, int n_out, int W, int H) { return pipe_slots ? pipe_slots : (long long)n_out * H * W < 500ll * 1000 * 1000 ? NSLOT : big_slots; }
// hc_pipeline_depth.  big batches: two slots, three while the hysteresis chain bounds the step (ChainWatch)
inline int pipeline_depth(bool pipeline, int pipe_slots, int big_slots, int n_out, int W, int H)
{
  if (!pipeline) return 1;
  const int n = pipeline_slots(pipe_slots, big_slots, n_out, W, H);
  return (n < NSLOT && !pipe_slots) ? 3 : n;
}

// What the hysteresis chain of a run did to the front kernel it ran beside, from timestamps of the runs themselves
// (recorded behind every pipelined run's front kernel and behind its last hysteresis launch).  update() is called
// when run i is complete: the chain of run i-1 ran beside the front kernel of run i, and all three events involved --
// end of front i-1, end of chain i-1, end of front i -- are complete.
//  * Two or three slots for big batches?  With two, the front kernel of run i+2 waits for the hysteresis of run i: while
//    that chain is the shorter of the two nothing waits, and a third slot only lets a second chain compete for the same
//    wave slots (-1 % at 1080p).  Where the chain outlasts the front kernel (8K: 30 dependent launches over 68 row tiles
//    and 4 column panels) the front kernels sit idle for the difference, and a third slot lets the next run start on
//    time.  Three runs in a row whose chain ended after the front kernel beside it -> a third slot ON TRIAL: kept if
//    the mean step of runs 7-10 with it is 3 % shorter than the last four steps without (8K x 3: -11 %, 8K grey -8 %,
//    256 frames of 1080p -5 %), otherwise given back, next trial after 64 runs, doubling; from three back to two after
//    16 runs in a row (doubling, up to 1024) whose chain ended first.
//  * One-wave or four-wave workgroups for k_front8?  One-wave workgroups take every slot a retiring wave leaves at once:
//    the front kernel gains 2-3 %, the hysteresis stream needs 40 % longer -- good while that stream has the time
//    (1080p grey: it ends 40 % of a front kernel early; +1.5 % frames/s), bad where it has none (BGR -> grey: -5 %).
//    By the smoothed share of the front kernel's time that the chain left unused: above 25 % -> one wave (1080p grey 41 %,
//    640 x 480 32 %, 4K 27 %; BGR -> grey 5 %), and back to four below 3 % (with one-wave workgroups the same streams
//    leave 17 %, 7 %, 15 %; BGR -> grey would fall 90 % behind).
struct ChainWatch {
  int pipe_slots = 0;  // HC_OPT_PIPELINE_SLOTS 2 / 3: that many slots whatever the batch size (0: by the rule)
  int chain_told = 0;  // diagnostics (HC_OPT_PIPELINE_SLOTS 20 / 21): +1 / -1 = every chain counts as ending after / before the next front kernel
  int big_slots = 2;   // slots of big pipelined batches: 2, or 3 while the hysteresis chain bounds the step
  bool front_one = false;  // the automatic choice: one-wave workgroups for k_front8 (mono / BGR, pipelined big batches)
  float slack_ema = 0.0f;  // share of a front kernel's time by which the previous run's hysteresis chain ended before it (smoothed)
  int chain_bound_runs = 0, chain_light_runs = 0, chain_light_needed = 16;
  float period_ms[4] = { 0, 0, 0, 0 }, period_two = 0.0f;  // the last four steps (front kernel end to front kernel end); their mean before the trial of a third slot
  int trial_runs = -1;                                      // >= 0: runs since the third slot was taken on trial
  int retry_wait = 0, retry_backoff = 64;                   // runs until the next trial after one that did not pay (doubling)

  // run i of a ring of nslot_use (2 or 3) slots is complete.  front_ms: front kernel i, end of the previous one to its end
  // (the step); lead_ms: end of chain i-1 -> end of front kernel i
  void update(unsigned long long i, int nslot_use, float front_ms, float lead_ms)
  {
    if (front_ms <= 0.0f) return;
    const bool outlasts = chain_told ? chain_told > 0 : lead_ms < 0.0f;
    period_ms[i & 3] = front_ms;
    const float period4 = 0.25f * (period_ms[0] + period_ms[1] + period_ms[2] + period_ms[3]);
    if (retry_wait > 0) --retry_wait;
    if (!pipe_slots) {
      if (nslot_use == 2 && big_slots == 2) {
        chain_bound_runs = outlasts ? chain_bound_runs + 1 : 0;
        if (chain_bound_runs >= 3 && i >= 5 && (retry_wait == 0 || chain_told)) {  // try a third slot
          period_two = period4;
          big_slots = 3;
          trial_runs = 0;
          chain_bound_runs = chain_light_runs = 0;
        }
      } else if (nslot_use == 3 && trial_runs >= 0) {  // the trial: ten runs, the last four measured
        if (++trial_runs >= 10) {
          trial_runs = -1;
          const bool better = chain_told ? chain_told > 0 : period4 < 0.97f * period_two;
          if (!better) {
            big_slots = 2;
            retry_wait = retry_backoff;
            retry_backoff = std::min(4096, 2 * retry_backoff);
          }
        }
      } else if (nslot_use == 3) {
        chain_light_runs = outlasts ? 0 : chain_light_runs + 1;
        if (chain_light_runs >= chain_light_needed) {
          big_slots = 2;
          chain_light_needed = std::min(1024, 2 * chain_light_needed);
          chain_bound_runs = chain_light_runs = 0;
        }
      }
    }
    const float slack = std::max(-1.0f, std::min(1.0f, lead_ms / front_ms));
    slack_ema = 0.75f * slack_ema + 0.25f * slack;
    if (!front_one && slack_ema > 0.25f) front_one = true;
    else if (front_one && slack_ema < 0.03f) front_one = false;
  }
};

// ---- the front path -----------------------------------------------------------------------------
// bits of the reference's stages a profiled interval covers (ProfRing::mark)
constexpr unsigned B_MONO = 1u << HC_STAGE_MONO, B_GAUSS = 1u << HC_STAGE_GAUSSIAN, B_GRAD = 1u << HC_STAGE_GRADIENT,
                   B_NMS = 1u << HC_STAGE_NMS, B_THR = 1u << HC_STAGE_THRESH, B_HYST = 1u << HC_STAGE_HYSTER;

// the caller's choices that shape the front path (hc_set_option, hc_set_tuning, hc_set_thresholds)
struct FrontOpts {
  int low = 10, high = 40;
  int nms_saturate = 0;
  int split = 2;        // Mode R front path: 2 = k_front8 (one kernel, 8 px per lane; default), 1 = k_blur + k_nms, 0 = the 4-px fused k_front
  int l2gradient = 0;   // Mode O: cv::Canny's L2gradient flag
  int aperture = 3;     // Mode O: cv::Canny's apertureSize (HC_OPT_APERTURE: 3 = k_front8o / k_front_o, 5 = k_front_o_ext; hc_canny_device also 7 and -1 = Scharr, per call)
  int call_lo = -1, call_hi = -1;  // >= 0 (hc_canny_device): the thresholds as the Mode O kernels compare them (canny_call_thresholds) instead of low / high
  int half_mode = -1;   // HC_OPT_FRONT_HALF: -1 automatic, 0 never, 1 whenever the buffers allow it
  int dense_mode = -1;  // HC_OPT_FRONT_DENSE: -1 automatic, 0 never, 1 every window
  int mx_mode = 0;      // HC_OPT_FRONT_MX: 1 = k_front_mx whenever the run allows it (opt-in: include/hipcanny.h)
  int wpb_mode = -1;    // HC_OPT_FRONT_WPB: -1 = by the slack of the hysteresis stream, 1 / 4 = fixed
  int dense_enter = 512, dense_leave = 384;  // HC_OPT_TEST_DENSE_ENTER / LEAVE (experiments)
  int chunk = 0;        // hc_set_tuning: rows per work item (0: by the rules)
  bool debug_taps = false;
};

struct FrontIn {
  int mode, C, W, H, RD, nstrips, per_channel, stage, n;
  View in, out;                      // the caller's views
  uintptr_t in_dy;                   // != 0: `in` / in_dy are the int16 dx / dy planes of cv::Canny's (dx, dy) overload
  View own_in, own_mono, own_out;    // the context's internal buffers (pitch and frame stride only)
  FrontOpts o;
  size_t dump_region;  // 0: the plain dump layout; otherwise four regions of this size (alloc_dump)
  bool piped;          // pipelined run (its hysteresis goes to the slot's own stream)
  int nslot_use;       // slots the pipelined runs rotate through
  bool front_one;      // ChainWatch's hint
  bool out_overlap;    // the output overlaps that of the previous, still pending run
  size_t wl_cap;       // tiles the slot's worklists and reason words hold (slot_wl_cap)
};

struct FrontPlan {
  const char *error = nullptr;  // HC_E_ARG with this text: nothing may be launched
  bool in_staged = false, out_staged = false;  // the caller's view goes through the internal buffer
  bool gray = false;    // 3-channel frames the front kernel cannot convert while loading: launch_gray first (stage MONO: into the output)
  View src{}, mono{}, dst{};  // what the kernels read / the one-channel frames / what they write (p: 0 = the internal buffer)
  int form = HC_FORM_FRONT_O;  // hc_last_run_info: one of HC_FORM_* (include/hipcanny.h); stays HC_FORM_FRONT_O when no front kernel runs
  bool prov = false;    // the front kernel writes the provisional map
  FrontParams fp{};     // complete but for the device pointers (in, planes, prov_out, dbg_blur, blur, dump areas, zero_words)
  size_t zeroed_words = 0;  // words of the slot's d_flags the front kernel zeroes (0: the host clears them)
  int waves = 0;        // waves per workgroup of k_front8 / k_front_mx (0: another kernel runs)
  unsigned mask = 0, mask_a = 0;  // reference stages the front launch covers; mask_a: k_blur's, when k_blur + k_nms run
};

// "stored u8 gradient > T" as thresholds on S = sumX^2+sumY^2 (gradient g = isqrt(S>>2)):
// wrapping variant: g in [256k+T+1, 256k+255] for k = 0,1,2  ->  S >= a[k] (and below 4*(256(k+1))^2);
// saturating variant: min(g,255) > T  ->  S >= a[0], never for T = 255.
inline void band_thresholds(int T, bool saturate, u32 a[3])
{
  for (int k = 0; k < 3; ++k) {
    const u64 g = 256ull * k + (u64)T + 1;
    a[k] = (u32)std::min<u64>(4ull * g * g, 0xFFFFFFFFull);
  }
  if (saturate && T >= 255) a[0] = 0xFFFFFFFFu;
}

// hc_canny_device's thresholds, as canny.cpp derives them from cv::Canny(img, edges, low, high, apertureSize, L2gradient)'s
// arguments: ordered; at aperture 7 both divided by 16 (the scale of its Sobel); with L2gradient min(32767, t) and then
// t * t for t > 0; floored.  lo / hi: those values.  k_lo / k_hi: what the kernels compare the magnitude with, "m > t" in
// int: the L1 thresholds clamped to 32767 (no L1 magnitude of any aperture on a u8 source reaches 32767 -- at most 24480,
// at aperture 5 -- so the clamp changes no result), the L2 ones as they are (at most 32767^2).
// false: a threshold is negative or not finite, or the aperture is none of 3, 5, 7, -1.
struct CallThresholds { long long lo, hi; int k_lo, k_hi; };
inline bool canny_call_thresholds(double low, double high, int aperture, bool l2, CallThresholds *t)
{
  if (aperture != 3 && aperture != 5 && aperture != 7 && aperture != -1) return false;
  if (!std::isfinite(low) || !std::isfinite(high) || low < 0.0 || high < 0.0) return false;
  if (low > high) std::swap(low, high);
  if (aperture == 7) { low /= 16.0; high /= 16.0; }
  if (l2) {
    low = std::min(32767.0, low); high = std::min(32767.0, high);
    if (low > 0.0) low *= low;
    if (high > 0.0) high *= high;
  }
  const double top = 9.0e18;  // (beyond every magnitude by far; keeps the conversion defined)
  t->lo = (long long)std::floor(std::min(low, top));
  t->hi = (long long)std::floor(std::min(high, top));
  t->k_lo = (int)(l2 ? t->lo : std::min<long long>(t->lo, 32767));
  t->k_hi = (int)(l2 ? t->hi : std::min<long long>(t->hi, 32767));
  return true;
}

#ifdef HC_LEGACY_FRONT
// rows per work item: about 16 rounds of the whole chip (8192 resident waves) when the batch allows it -- the tail of a
// launch is one work item long, measured optimum 68-135 rows at 1024 frames -- but never runs shorter than 64 rows
// (each run repeats a 4-row warm-up)
inline int pick_run_rows(long units, int H, int want_rows)
{
  if (want_rows > 0) return std::min(std::max(want_rows, 2), H);
  const long nch = std::min<long>(std::max<long>((16 * 8192 + units - 1) / units, 1), std::max(1, H / 64));
  return (int)((H + nch - 1) / nch);
}
#endif

// does the caller's output view go through the internal buffer?  (the kernels store dwords)
inline bool out_view_staged(const View &out) { return !aligned4(out.p, out.pitch, out.fs); }

// groups of front forms (HC_FORM_*, include/hipcanny.h) that share a rule
inline bool form_8px(int f) { return f == HC_FORM_FRONT8 || f == HC_FORM_FRONT8O || f == HC_FORM_FRONT8_HALF; }
inline bool form_o_ext(int f) { return f == HC_FORM_O_APERTURE5 || f == HC_FORM_O_GRADIENTS || f == HC_FORM_O_APERTURE7 || f == HC_FORM_O_SCHARR; }  // k_front_o_ext's
inline bool form_o_4px(int f) { return f == HC_FORM_FRONT_O || form_o_ext(f); }
inline bool form_zeroes_flags(int f) { return form_8px(f) || f == HC_FORM_FRONT_MX; }  // these kernels zero the run's hysteresis flag words on their way in

inline int front_out_frames(const FrontIn &in) { return in.per_channel ? 3 * in.n : in.n; }  // output frames (= bit-plane frames)
// Mode O forms of k_front_o_ext: caller-given gradients (HC_FORM_O_GRADIENTS), or aperture 5, 7 or -1 on u8 frames
// (HC_FORM_O_APERTURE5 / HC_FORM_O_APERTURE7 / HC_FORM_O_SCHARR)
inline bool front_o_ext(const FrontIn &in) { return in.mode == HC_MODE_O && (in.in_dy != 0 || in.o.aperture == 5 || in.o.aperture == 7 || in.o.aperture == -1); }
// the fused kernel converts BGR while loading (needs whole 12-byte pixel groups inside each row)
inline bool whole_bgr_groups(const View &src, int W) { return src.pitch >= round_up((size_t)W, 4) * 3; }
inline bool fuses_bgr(const FrontIn &in, const FrontPlan &P) { return in.C == 3 && in.stage == HC_STAGE_HYSTER && whole_bgr_groups(P.src, in.W); }

// Staging: which of the caller's views go through the internal buffers, and where stage 0 (grey) runs.
inline void stage_views(const FrontIn &in, FrontPlan &P)
{
  const FrontOpts &o = in.o;
  const int W = in.W, H = in.H, C = in.C;
  const bool hyster = in.stage == HC_STAGE_HYSTER, grad_in = in.in_dy != 0, ext = front_o_ext(in);
  // unaligned caller buffers go through the internal pitched ones
  // (mode O on 3-channel data reads whole 12-byte groups of 4 pixels: a tighter caller pitch is staged as well; so are
  // rows that do not hold whole 8-pixel groups when the 8-px front kernels are to run -- k_front8 / k_front8o load 8 or
  // 24 bytes per lane and row: tight rows of a width that is not a multiple of 8.  Round 2 fell back to the 4-px kernels
  // for those; one copy through the internal pitched buffer keeps every frame on the one-kernel path)
  // (k_front_o_ext on u8 frames reads whole 4-pixel groups, in every channel count)
  const bool wants8 = hyster && o.split == 2 && (in.mode == HC_MODE_R || C == 1) && !ext;
  // (the front kernels address the rows of a frame with 32-bit offsets: a view whose height x pitch reaches 4 GiB -- a few
  // columns of a huge parent -- is staged as well instead of being refused by their launchers)
  P.in_staged = !grad_in && (!aligned4(in.in.p, in.in.pitch, in.in.fs) || reaches_4g(H, in.in.pitch)
                             || (in.mode == HC_MODE_O && (C == 3 || ext) && in.in.pitch < round_up((size_t)W, 4) * C)
                             || (wants8 && in.in.pitch < round_up((size_t)W, 8) * (size_t)C));
  P.src = P.in_staged ? View{ 0, in.own_in.pitch, in.own_in.fs } : in.in;
  P.out_staged = out_view_staged(in.out);
  P.dst = P.out_staged ? View{ 0, in.own_out.pitch, in.own_out.fs } : in.out;
  // stage 0 (cannyEdgeH.cu:214-227); 1-channel input skips it (the reference's mono path is broken, SURVEY §3 ii)
  if (in.per_channel && !whole_bgr_groups(P.src, W)) { P.error = "per-channel mode needs an input pitch of at least 3 * round_up(width, 4) bytes"; return; }
  P.gray = C == 3 && !fuses_bgr(in, P) && !grad_in;
  P.mono = (P.gray && in.stage != HC_STAGE_MONO) ? View{ 0, in.own_mono.pitch, in.own_mono.fs } : P.src;
}

// The form HC_OPT_FRONT_SPLIT, the mode and the source ask for; choose_form looks at a HC_FORM_FRONT8 run more closely.
// Mode R front path: k_front8 reads whole 8-pixel groups (8 or 24 bytes per lane and row), the 4-px kernels 4-pixel
// groups.  (Rows too tight for the 8-px kernels were staged above -- wants8 covers every case that asks for HC_FORM_FRONT8
// or HC_FORM_FRONT8O -- so no run falls back to another form for its pitch; tests/cpp/plan_driver.cpp checks it.)
// Mode O: k_front8o for one-channel sources, the 4-px k_front_o for 3-channel ones or when HC_OPT_FRONT_SPLIT asks for a
// 4-px form
// (Narrow frames: k_front8's HALF form, choose_form.  Round 2 sent 640-column batches to k_blur + k_nms instead.)
inline int asked_form(const FrontIn &in)
{
  if (front_o_ext(in)) return in.in_dy != 0 ? HC_FORM_O_GRADIENTS : in.o.aperture == 7 ? HC_FORM_O_APERTURE7 : in.o.aperture == -1 ? HC_FORM_O_SCHARR : HC_FORM_O_APERTURE5;
  if (in.mode != HC_MODE_R) return (in.C == 1 && in.o.split == 2) ? HC_FORM_FRONT8O : HC_FORM_FRONT_O;
  return in.o.split;  // HC_FORM_FRONT8 / HC_FORM_SPLIT / HC_FORM_FRONT4 are HC_OPT_FRONT_SPLIT's values
}

// Does the front kernel write the provisional map?  By the inputs alone, so it is settled before the form is.
// Pipelined mode: k_nms / k_front_o also write the strong pixels as 255 into the output (4 px per lane: whole
// dwords need W % 4 == 0), so that the hysteresis, which runs beside the next run's bandwidth-hungry k_blur, only
// rewrites the 16-pixel groups it changes instead of streaming out the whole map (+8 % end to end; without the
// overlap the extra stores of the VALU-bound kernel cost more than the hysteresis saves).
// Not when this run's output overlaps the previous run's (a caller that keeps one output buffer): that run's
// hysteresis may still be patching it, and a late patch would survive into this run's map.
// (k_front_o_ext writes no provisional map: its runs give the hysteresis the whole map to write)
// (nor into an output view whose height x pitch reaches 4 GiB: the front kernels place the provisional rows with 32-bit
// offsets, which would wrap -- row 1024 of a 4 MiB pitch onto row 0; the hysteresis, with 64-bit offsets, writes that map)
inline bool front_writes_prov(const FrontIn &in, const View &dst, int asked)
{
  const bool f8 = asked == HC_FORM_FRONT8 || asked == HC_FORM_FRONT8O;
  return in.piped && !in.out_overlap && !front_o_ext(in) && !reaches_4g(in.H, dst.pitch)
         && (f8 ? in.W % 8 == 0 : (in.W % 4 == 0 && (asked == HC_FORM_SPLIT || in.mode == HC_MODE_O)));
}

// waves a run of rows of the 8-px kernels takes: one per (output frame, strip of 496 columns); HALF form (narrow frames):
// the (frame, 240-column half-strip) units of a run of rows are dealt to half-waves in pairs -- 640 columns: 1.5 waves
// instead of 2 -- three times that in per-channel mode
inline long front8_waves_per_run(const FrontIn &in, bool half)
{
  if (!half) return (long)front_out_frames(in) * front8_strips(in.W);
  return (((long)in.n * front8_half_strips(in.W) + 1) / 2) * (in.per_channel ? 3 : 1);
}

// The form that runs (needs P.src, P.dst, P.prov and P.fp.bgr).  Whatever is not HC_FORM_FRONT8 runs as asked.
inline int choose_form(const FrontIn &in, const FrontPlan &P, int asked)
{
  if (asked != HC_FORM_FRONT8) return asked;
  const FrontOpts &o = in.o;
  const int W = in.W, H = in.H;
  const size_t sp = P.src.pitch, sfs = P.src.fs, dp = P.dst.pitch, dfs = P.dst.fs;
  const bool mx_asked = o.mx_mode == 1 && P.fp.bgr == 0 && !in.per_channel;
  if (in.dump_region && o.half_mode != 0 && !mx_asked) {  // (HC_OPT_FRONT_MX 1 goes first)
    // HALF form: when that needs fewer waves and the lane offsets fit
    const long per = in.per_channel ? 3 : 1;
    const size_t R = in.dump_region;
    const bool fits = sfs + 32768 <= R && per * sizeof(u32) * (size_t)in.RD * H + 4096 <= R && (!P.prov || per * dfs + 16384 <= R)
                      && (unsigned long long)sfs + (unsigned long long)H * sp < (1ull << 32) && (!P.prov || (unsigned long long)per * dfs + (unsigned long long)H * dp < (1ull << 32));
    if ((front8_waves_per_run(in, true) < front8_waves_per_run(in, false) || o.half_mode == 1) && fits) return HC_FORM_FRONT8_HALF;
  }
  // k_front_mx (blur and Sobel on the matrix pipe): one-channel frames of Mode R, on request (HC_OPT_FRONT_MX)
  if (P.fp.bgr == 0 && o.mx_mode == 1 && !reaches_4g(H, sp) && sp >= round_up((size_t)W, 4) && (!P.prov || W % 8 == 0)) return HC_FORM_FRONT_MX;
  return HC_FORM_FRONT8;
}

// what the flag-zeroing forms share: the words of the slot's d_flags the kernel zeroes (every tile shape has at least 16
// rows per tile), and k_front8's dense path
inline void plan_zeroing_and_dense(const FrontIn &in, FrontPlan &P)
{
  const FrontOpts &o = in.o;
  FrontParams &fp = P.fp;
  P.zeroed_words = run_flag_words(std::min(in.wl_cap, slot_wl_cap((size_t)front_out_frames(in), in.H, in.RD)));
  fp.zero_count = (u32)P.zeroed_words;
  // dense path of k_front8 (wave-wide NMS): enter above 512 half-lanes per window of 768, leave below 384.  Both paths
  // count the half-lanes above the low threshold in the window's rows 2 .. H-3 only (the zero padding makes the frame's
  // first and last two rows candidates across the whole width).  Measured (profiles/r10_dense/, 1080p, 1024 frames):
  // of the interior windows 1.1 % (natural), 1.0 % (natural-B), 2.1 % (blend) and none (noise) count 320 .. 512, so the
  // thresholds decide little; lowering dense_enter from 512 to 192 (leave at 3/4) raises the front kernel on natural
  // frames step by step from 2.12 to 2.18 ms, and no lower value reached the rotation's 302.9 k frames/s at 512 (192:
  // 301.2 k, 256: 300.0 k, 320: 300.7 k, 384: 302.1 k, 448: 302.1 k).  On noise only 192 differs (3.26 -> 3.16 ms): a run's first window has two rows of its own and counts
  // 248, so with any higher value the second window still takes the queue path.
  // (k_front_mx has no dense path and reads neither value; its plans have always carried them and still do)
  fp.dense_enter = o.dense_mode == 0 ? 0x7FFFFFFF : o.dense_mode == 1 ? -1 : o.dense_enter;
  fp.dense_leave = o.dense_mode == 0 ? 0x7FFFFFFF : o.dense_mode == 1 ? -1 : o.dense_leave;
}

// k_front8, its HALF form and k_front8o: strips of 496 columns, runs of 6 * windows - 4 rows
inline void cut_front8_runs(const FrontIn &in, FrontPlan &P)
{
  const FrontOpts &o = in.o;
  FrontParams &fp = P.fp;
  const int H = in.H;
  plan_zeroing_and_dense(in, P);
  fp.nstrips = front8_strips(in.W);
  if (P.form == HC_FORM_FRONT8_HALF) { fp.half = 1; fp.nhalf = front8_half_strips(in.W); }
  const long waves_per_chunk = front8_waves_per_run(in, P.form == HC_FORM_FRONT8_HALF);
  // Run length.  Every run repeats an 8-row warm-up, so long runs are cheaper -- measured optimum 110-180 rows at 1024
  // frames, provided the runs tile the frame evenly (a last run of a few rows pays the warm-up for nothing): the frame
  // is cut into round(H / 120) equal runs.  A small batch is cut into shorter runs instead, down to 8 rows, where the
  // warm-up doubles the work but one frame still spreads over 540 waves (3072 waves of this kernel are resident).
  int rows;
  if (o.chunk) rows = std::min(std::max(o.chunk, 2), H);
  else {
    const long units = waves_per_chunk;
    long nch = std::max<long>(1, (H + 60) / 120);
    if (units * nch < 3072) nch = std::min<long>((3072 + units - 1) / units, std::max(1, H / 8));  // (spread over 2048 / 1536 / 1024 waves instead: no better, profiles/r03/experiments.md)
    rows = (int)((H + nch - 1) / nch);
  }
  const int windows = std::max(1, (rows + 4 + 5) / 6);
  fp.run_rows = front8_run_rows(windows);
  fp.nchunks = (H + fp.run_rows - 1) / fp.run_rows;
  fp.total_items = (int)(waves_per_chunk * fp.nchunks);
}

// k_front_mx: strips of 216 columns, runs of any length (blocks of 16 rows)
inline void cut_front_mx_runs(const FrontIn &in, FrontPlan &P)
{
  const FrontOpts &o = in.o;
  FrontParams &fp = P.fp;
  const int H = in.H;
  plan_zeroing_and_dense(in, P);
  fp.nstrips = front_mx_strips(in.W);
  const long units = (long)front_out_frames(in) * fp.nstrips;
  // a run of n blocks covers 16 n - 4 rows and costs about one block more to start (workgroup launch, prologue: 0.2 ms
  // of a 1024-frame launch in runs of 124 rows, profiles/r04/mx_ablation.txt): the run count that needs the fewest
  // blocks in all, among those that give every wave slot of the chip (3072) six runs or more where the frame allows
  long nch;
  if (o.chunk) nch = std::max<long>(1, (H + o.chunk - 1) / o.chunk);
  else {
    const long hi = std::max<long>(1, (H + 11) / 12);
    const long lo = std::min<long>(hi, std::max<long>(1, (6 * 3072 + units - 1) / units));
    long best = -1, best_cost = 0;
    for (long k = lo; k <= std::min<long>(hi, lo + 24); ++k) {
      const long rows = (H + k - 1) / k, runs = (H + rows - 1) / rows, last = H - rows * (runs - 1);
      const long cost = ((rows + 4 + 15) / 16 + 1) * (runs - 1) + (last + 4 + 15) / 16 + 1;
      if (best < 0 || cost < best_cost) { best = k; best_cost = cost; }
    }
    nch = best;
  }
  fp.run_rows = (int)((H + nch - 1) / nch);
  fp.nchunks = (H + fp.run_rows - 1) / fp.run_rows;
  fp.total_items = (int)(units * fp.nchunks);
}

// k_front_o, and k_front_o_ext with its strips and work split (a 6-row warm-up for aperture 5, 8 rows for 7, 4 for Scharr, 2 for gradients):
// strips of 248 columns (FrontIn::nstrips), long chunks (no LDS slab, 4-row warm-up)
inline void cut_front_o_chunks(const FrontIn &in, FrontPlan &P)
{
  FrontParams &fp = P.fp;
  const int H = in.H;
  // rows per work item: hc_set_tuning's number (any value >= 1: these kernels have no window to fill, unlike the 8-px
  // forms, whose runs are 2 rows at least), or about 12288 items per launch in chunks of 16 rows or more
  const long units = (long)front_out_frames(in) * in.nstrips;
  const int per_strip = (int)std::max<long>(1, std::min<long>((12288 + units - 1) / units, (H + 15) / 16));
  fp.chunk_rows = in.o.chunk ? std::min(std::max(in.o.chunk, 1), H) : (H + per_strip - 1) / per_strip;
  fp.nchunks = (H + fp.chunk_rows - 1) / fp.chunk_rows;
  fp.total_items = front_out_frames(in) * fp.nstrips * fp.nchunks;
  if (!front_o_ext(in) && P.src.pitch < round_up((size_t)in.W, 4) * (size_t)in.C) P.error = "mode O needs an input pitch of at least round_up(width, 4) * channels";
}

#ifdef HC_LEGACY_FRONT
// k_front (Mode R, fused, 4 px per lane): a wave marches through `subchunks` sub-chunks of 24 blur rows (run of 24*m - 4
// output rows).  Longer runs amortise the 8-row warm-up; shorter runs give more work items (small batches).
inline void cut_front4_runs(const FrontIn &in, FrontPlan &P)
{
  FrontParams &fp = P.fp;
  const int H = in.H, n_out = front_out_frames(in);
  int m = in.o.chunk ? (in.o.chunk + 4 + 23) / 24 : 0;
  if (m == 0) {
    m = 3;
    while (m > 1 && (long)n_out * in.nstrips * ((H + front_run_rows(m) - 1) / front_run_rows(m)) < 24576) --m;
  }
  fp.subchunks = m; fp.run_rows = front_run_rows(m);
  fp.nchunks = (H + fp.run_rows - 1) / fp.run_rows;
  fp.total_items = n_out * fp.nstrips * fp.nchunks;
}

// k_blur + k_nms through the blur plane: each with a work split of its own
inline void cut_split_runs(const FrontIn &in, FrontPlan &P)
{
  FrontParams &fp = P.fp;
  const int H = in.H, n_out = front_out_frames(in);
  const int rows = pick_run_rows((long)n_out * in.nstrips, H, in.o.chunk);
  fp.run_rows = (rows + 1) & ~1;  // k_blur walks rows in pairs
  fp.nchunks = (H + fp.run_rows - 1) / fp.run_rows;
  fp.total_items = n_out * fp.nstrips * fp.nchunks;
  fp.run_rows_b = rows;
  fp.nchunks_b = (H + rows - 1) / rows;
  fp.total_items_b = n_out * fp.nstrips * fp.nchunks_b;
}
#endif

// thresholds as the form's kernel compares them, and the reference stages its launch covers
inline void plan_thresholds_and_masks(const FrontIn &in, FrontPlan &P)
{
  const FrontOpts &o = in.o;
  FrontParams &fp = P.fp;
  if (in.mode == HC_MODE_O) {
    // cv::Canny: plain thresholds on the L1 magnitude
    fp.a_lo[0] = (u32)o.low; fp.a_hi[0] = (u32)o.high;
    fp.l2gradient = o.l2gradient;
    if (o.l2gradient) {  // canny.cpp: thresholds capped at 32767 (hc_set_thresholds) and squared; the magnitude is dx^2 + dy^2
      fp.a_lo[0] = (u32)o.low * (u32)o.low;
      fp.a_hi[0] = (u32)o.high * (u32)o.high;
    }
    if (o.call_lo >= 0 && o.call_hi >= 0) { fp.a_lo[0] = (u32)o.call_lo; fp.a_hi[0] = (u32)o.call_hi; }  // hc_canny_device: squared already where L2
    // cv::Canny has no blur stage; given gradients leave NMS + thresholds only (GRADIENT did not run)
    P.mask = (in.in_dy != 0 ? 0u : B_GRAD) | B_NMS | B_THR;
    return;
  }
  band_thresholds(o.low, o.nms_saturate != 0, fp.a_lo);
  band_thresholds(o.high, o.nms_saturate != 0, fp.a_hi);
  fp.wrap_limit = o.nms_saturate ? 0xFFFFFFFFu : 262144u;
  const unsigned b_mono = fuses_bgr(in, P) ? B_MONO : 0u;  // stage 0 fused into the blur's load (per-channel mode has no grey stage)
  const bool split = P.form == HC_FORM_SPLIT;
  P.mask = split ? B_GRAD | B_NMS | B_THR : b_mono | B_GAUSS | B_GRAD | B_NMS | B_THR;
  P.mask_a = split ? b_mono | B_GAUSS : 0u;
}

// waves per workgroup of k_front8 (both forms) and k_front_mx; every other kernel has one shape (P.waves stays 0)
inline void plan_front_waves(const FrontIn &in, FrontPlan &P)
{
  const FrontOpts &o = in.o;
  FrontParams &fp = P.fp;
  if (P.form == HC_FORM_FRONT8 || P.form == HC_FORM_FRONT8_HALF) {
    // one-wave workgroups: pipelined big batches with the provisional map, mono / BGR (the per-channel form is three waves, one per channel)
    // (small batches, whose four chains overlap anyway: from 0.12 G pixels per run -- 64 frames of 1080p +3.5 %, 128 frames
    //  +4.5 %; 4 to 32 frames -3 to -6 %: tools/experiments/exp_small_wpb.sh)
    const bool auto_one = in.nslot_use < NSLOT ? in.front_one : (long long)front_out_frames(in) * in.W * in.H >= 120ll * 1000 * 1000;
    fp.one_wave = (P.prov && !in.per_channel && (o.wpb_mode == 1 || (o.wpb_mode < 0 && auto_one))) ? 1 : 0;
    P.waves = in.per_channel ? 3 : fp.one_wave ? 1 : 4;
  } else if (P.form == HC_FORM_FRONT_MX) {
    // (its waves are independent too: one-wave workgroups beside the hysteresis, -3.5 % there, four-wave ones alone; HC_OPT_FRONT_WPB 1 / 4 fixes it)
    fp.one_wave = (o.wpb_mode == 1 || (o.wpb_mode < 0 && P.prov)) ? 1 : 0;
    P.waves = fp.one_wave ? 1 : 4;
  }
}

// A run's front path: staging, then the form, then the work split, thresholds and workgroup shape of that form.
inline FrontPlan plan_front(const FrontIn &in)
{
  FrontPlan P;
  stage_views(in, P);
  if (P.error || in.stage != HC_STAGE_HYSTER) return P;

  FrontParams &fp = P.fp;
  fp.bgr = in.per_channel ? 2 : fuses_bgr(in, P) ? 1 : 0; fp.in_pitch = P.mono.pitch; fp.in_frame_stride = P.mono.fs; fp.RD = in.RD; fp.W = in.W; fp.H = in.H;
  fp.nstrips = in.nstrips; fp.nframes = front_out_frames(in);
  const int asked = asked_form(in);
  P.prov = front_writes_prov(in, P.dst, asked);
  P.form = choose_form(in, P, asked);
  if (P.prov) { fp.prov_pitch = (u32)P.dst.pitch; fp.prov_fs = P.dst.fs; }
  if (in.o.debug_taps && P.form != HC_FORM_SPLIT) { fp.dbg_pitch = (u32)in.own_out.pitch; fp.dbg_fs = in.own_out.fs; }  // own_out.pitch: the width if that is a multiple of 16, else padded to 256
  switch (P.form) {
  case HC_FORM_FRONT8: case HC_FORM_FRONT8_HALF: case HC_FORM_FRONT8O: cut_front8_runs(in, P); break;
  case HC_FORM_FRONT_MX: cut_front_mx_runs(in, P); break;
  case HC_FORM_FRONT_O: case HC_FORM_O_APERTURE5: case HC_FORM_O_GRADIENTS: case HC_FORM_O_APERTURE7: case HC_FORM_O_SCHARR: cut_front_o_chunks(in, P); break;
#ifdef HC_LEGACY_FRONT
  case HC_FORM_FRONT4: cut_front4_runs(in, P); break;
  case HC_FORM_SPLIT: cut_split_runs(in, P); break;
#endif
  default: P.error = "this library is built without the round-1 front kernels (HC_OPT_FRONT_SPLIT 1 / 0: libhipcanny_legacy.so)"; break;
  }
  if (P.error) return P;
  plan_thresholds_and_masks(in, P);
  plan_front_waves(in, P);
  return P;
}

// ---- the hysteresis schedule ----------------------------------------------------------------------
// hc_set_tuning and the HC_OPT_TEST_HYST_* hooks
struct HystOpts {
  int launches = 6;           // launches queued per run at least (hc_set_tuning)
  bool launches_set = false;  // hc_set_tuning called: queue exactly that many launches
  int late_grid = 0;          // tests (HC_OPT_TEST_HYST_LATE_GRID): workgroups of the hysteresis launches >= 1
  bool loop = true;           // small runs: one looping hysteresis launch (HC_OPT_TEST_HYST_LOOP 0 turns it off)
  // HC_HYST_DIAG (per-launch counters for hc_hysteresis_stats; slows the launches), HC_HYST_GEOM (hysteresis workgroup shape, e.g. "32x8")
  bool diag = false;
  int geom = 0;
};

struct HystPlan {
  int level = 0;                    // tile height level: waves = base shape's waves << level (HystHistory::obs index)
  int tile_rows = 0, waves = 0;     // rows per wave, waves per workgroup
  int nrtiles = 0, npanels = 0;     // row tiles per frame, column panels
  int K = 0;                        // launches queued (rounds of the looping launch)
  size_t wl_stride = 0;             // tiles of the run
  bool fits = true;                 // wl_stride <= the slot's wl_cap
  bool clear = true;                // the host must zero run_flag_words(wl_stride) words first (the front kernel zeroed too few)
  bool loop = false;                // all K rounds in one launch (k_hyst_loop)
  int lists0 = 0;                   // the list scheme the run started with (diagnostics)
  bool mixed = false;               // per-tile launches, then lists (lists[] = 0 .. 0, 2, 1 .. 1)
  int test_grid = 0;                // HC_OPT_TEST_HYST_LATE_GRID > 0: the grid of every launch, continuation rounds included
  uint8_t lists[MAX_HYST_LAUNCHES] = { 0 };  // per launch: HystParams::lists
  int late_grid[MAX_HYST_LAUNCHES] = { 0 };  // per launch: HystParams::late_grid (sized from the last run's list unless test_grid)
  bool served_list(int k) const { return lists[k] == 1 && k > 0; }
  int hist_grid(int k) const { return test_grid ? 0 : late_grid[k]; }  // the grid that was sized from the last run's list (0: none)
};

// what finished runs teach the next plan
struct HystHistory {
  int obs[3] = { 0, 0, 0 };       // hysteresis launches the last runs needed with base_waves << i waves per workgroup (0: not seen)
  int obs_base = 0, obs_rows = 0;  // the base shape those observations belong to
  int need_rows = 0;  // launches that found work in recent runs (continuation rounds included) x rows per tile: how far changes travelled
  u32 wl_prev[MAX_HYST_LAUNCHES + 1] = { 0 };  // worklist lengths of the last finished run's launches
  size_t wl_prev_tiles = 0;                    // ... and its tile count (0: none / not a wide-frame run)
  int last_work_launches = 0;
  bool lists_last = false;  // the last run used the worklist scheme

  // a run has reached its fixpoint.  work: launches that found work, continuation rounds included (+ 1 when the queued
  // launches sufficed); wl_counts: MAX_HYST_LAUNCHES + 1 list lengths as the QUEUED launches left them
  void finished(const HystPlan &p, int work, const u32 *wl_counts)
  {
    last_work_launches = work;
    // worklist lengths of this run's launches (wide frames): the next run of the same shape sizes its grids by them
    wl_prev_tiles = (p.npanels > 1 || p.lists[p.K - 1]) ? p.wl_stride : 0;
    for (int k = 0; k <= MAX_HYST_LAUNCHES; ++k) wl_prev[k] = wl_counts[k];
    need_rows = std::max(work * p.tile_rows * p.waves, need_rows - 32);  // follows the content up at once, down slowly
    // launches this run needed at its tile height (plan_hyst picks the next runs' height from these)
    if ((p.waves >> p.level) != obs_base || p.tile_rows != obs_rows) return;
    const int o = obs[p.level];
    // the content changed: what was seen at the other heights no longer holds
    if (o && (work * 10 > o * 13 + 20 || work * 10 < o * 7 - 20)) obs[0] = obs[1] = obs[2] = 0;
    obs[p.level] = work;
  }
};

// n: output frames; small_tiles: the run is pipelined (its hysteresis runs beside the next front kernel);
// zeroed_words: what the front kernel zeroes of the slot's d_flags (FrontPlan::zeroed_words)
inline HystPlan plan_hyst(int RD, int H, int n, bool small_tiles, const HystOpts &o, HystHistory &h, size_t wl_cap, size_t zeroed_words)
{
  HystPlan p;
  // one workgroup per (frame, tile of waves x tile_rows rows); the geometry follows the row width
  hyst_tile_geometry(o.geom, small_tiles, (long)n * H, H, &p.tile_rows, &p.waves);
  // Adaptive tile height: a launch carries a change across one tile boundary, so frames whose weak edges wind through
  // many tiles need many launches.  The library remembers how many launches the runs needed with the base shape and
  // with twice / four times its waves (HystHistory::obs, forgotten when the content changes): above 20
  // launches the next taller shape is tried -- and kept only if it needs fewer than 60 % of the launches.  Mode O frames:
  // 24 launches with 64-row tiles, 5 with 128 rows: taller (501 against 480 k frames/s).  BGR frames blended into grey:
  // 25 either way, their chains wind around the tile boundaries whatever the height: the small workgroups, which find
  // room beside the front kernel more easily, and the worklists (255 against 224 k frames/s with 4-wave tiles).
  // (Round 2's first rule went by rows -- launches x tile height -- alone: it kept the BGR stream on tall tiles, and
  // made the Mode O stream flip between the two shapes every few runs, each flip a host-side continuation.)
  const int base_waves = p.waves;
  if (base_waves != h.obs_base || p.tile_rows != h.obs_rows) {  // another base shape (batch size, plain / pipelined): start over
    h.obs_base = base_waves; h.obs_rows = p.tile_rows;
    h.obs[0] = h.obs[1] = h.obs[2] = 0;
  }
  int lvl = 0;
  while (lvl < 2 && (base_waves << (lvl + 1)) <= 8) {
    const int cur = h.obs[lvl], nxt = h.obs[lvl + 1];
    if (cur <= 20) break;                  // unknown (0) or few enough
    if (nxt != 0 && nxt * 5 > cur * 3) {  // the taller tiles did not pay
      // (frames of several panels: the tallest then -- an 8K grey stream whose weak edge wobbles along a tile boundary
      // needs 53 launches at every height, and runs them faster on a quarter of the tiles: 21.1 against 16.5 k frames/s)
      if (RD > 64) while (lvl < 2 && (base_waves << (lvl + 1)) <= 8) ++lvl;
      break;
    }
    ++lvl;
  }
  p.waves = base_waves << lvl;
  p.level = lvl;
  const int tile = p.tile_rows * p.waves;
  p.nrtiles = (H + tile - 1) / tile;
  p.npanels = (RD + 63) / 64;
  // launches queued per run: the user's number, or by default enough for an edge that crosses every row tile of a
  // tall frame (later launches exit at once after convergence; beyond the queue, hc_sync continues from the host)
  // (one more than the tiles an edge can cross monotonically: the last queued launch must find nothing to do, or the host
  // continues in hc_sync -- which stalls a pipelined stream of runs)
  const int need = (h.need_rows + tile - 1) / tile;
  int K = std::min(MAX_HYST_LAUNCHES, std::max(std::max(o.launches, p.nrtiles + p.npanels + 1), need + 2));
  // One or a few frames per call, not pipelined (the reference's pattern): every queued launch that finds nothing to do
  // still costs ~5 us of pure latency, so only what the last runs needed is queued, + 2; frames that need more are
  // finished by the host-side continuation (cheap here: nothing else is in flight).
  if (!small_tiles && (long)n * H < 128 * 1024 && h.need_rows > 0) K = std::min(K, std::max(4, need + 2));
  // ... and in a pipelined stream whose needs are known, not the worst case of an edge down the whole frame (68 row tiles
  // at 8K: 70 launches queued, 50 of them idle at ~5 us each on the hysteresis stream) but what the last runs needed, + 4;
  // a frame that needs more is finished by the continuation, and the estimate follows it at once
  if (small_tiles && h.need_rows > 0) K = std::min(K, std::max(6, need + 4));
  // (a few frames per run, pipelined: the step is the host's time to queue the run -- 75 us for ~25 API calls -- so every
  // launch that is not needed counts)
  if (small_tiles && h.need_rows > 0 && (long)n * H < 128 * 1024) K = std::min(K, std::max(4, need + 2));
  if (o.launches_set) K = o.launches;
  p.K = K;
  // worklists of launches >= 1: counts and reason words live behind the launch flags and are zeroed with them
  p.wl_stride = (size_t)n * p.nrtiles * p.npanels;
  p.fits = p.wl_stride <= wl_cap;
  if (!p.fits) return p;
  p.clear = zeroed_words < run_flag_words(p.wl_stride);
  // Worklists or a workgroup per tile in every launch (k_hyst)?  Lists where the step follows the hysteresis chain:
  // frames wider than one panel -- unless they are dense (the last run visited more than 60 % of the tiles in launch 1:
  // noise; camera-like frames: a third; the front kernel, which bounds such streams, loses less to a hysteresis that is
  // spread over it: 33.6 against 30.8 k frames/s on 4K noise) -- and one-panel streams whose runs need 20 launches or more
  // (BGR frames blended into grey: 25 launches, 205 -> 222 k frames/s; the 16 launches of 1080p grey frames fit inside
  // the front kernel's time, and there the lists cost 2 %).
  bool lists;
  if (o.late_grid) lists = o.late_grid > 0;
  else if (p.npanels > 1) lists = !(h.wl_prev_tiles == p.wl_stride && (size_t)h.wl_prev[1] * 5 > p.wl_stride * 3);
  else lists = h.last_work_launches >= 20 || (h.lists_last && h.last_work_launches >= 14);
  h.lists_last = lists;
  p.lists0 = lists ? 1 : 0;
  p.test_grid = std::max(o.late_grid, 0);
  // The other streams: a workgroup per tile for launches 0 and 1 -- which do most of the work, and whose idle workgroups
  // keep the hysteresis spread over the front kernel it runs beside -- then lists for the tail of launches that follow a
  // few long edges through the frame (launch 2 still starts every tile, and writes the first list): 1080p grey 394 -> 405 k
  // frames/s, 256 frames per run 307 -> 317 k; with the lists from launch 1 on: 400 k, from launch 4: 404 k.  (The list
  // streams above keep their lists from launch 1: BGR 259 against 252 k, 8K x 3 8.76 against 8.64 k; 4K would gain 2 %.)
  constexpr int MIXED_FROM = 2;  // first launch of a mixed-schedule run that works from lists
  p.mixed = !lists && !o.late_grid && small_tiles;
  // A small run (a few frames): all K rounds in one launch, device-wide barriers between them (k_hyst_loop) -- K host
  // calls and K trips through the command processor fewer per run; a run it cannot finish (its workgroups not resident
  // together, or more rounds needed than queued) is continued by finish_slot like any other.
  // (not beside other runs: in the pipelined small batches the rounds' barriers -- ~10 us each, with the waiting workgroups
  // resident -- cost more than the launches they replace: 8 frames per run 0.147 against 0.117 ms per call; one frame per
  // call, the reference's pattern: 0.150 against 0.168 ms)
  p.loop = o.loop && !small_tiles && !lists && !o.late_grid && !o.diag && p.npanels == 1 && RD == 64 && p.wl_stride <= (size_t)HYST_LOOP_MAX_TILES
           && hyst_shape_loops(p.tile_rows, p.waves);
  if (p.loop) p.mixed = false;
  for (int k = 0; k < K; ++k) {
    p.lists[k] = (uint8_t)(p.mixed ? (k < MIXED_FROM ? 0 : k == MIXED_FROM ? 2 : 1) : lists ? 1 : 0);
    // worklist scheme, launches >= 1: a workgroup per list entry.  Grid: twice what the last run of this shape listed for
    // the launch (entries beyond the grid wait a launch: a dense frame would need several launches more); without such
    // a run, launch_hyst's schedule by the tile count
    p.late_grid[k] = p.test_grid;
    if (!p.loop && p.lists[k] == 1 && !p.test_grid && k > 0 && h.wl_prev_tiles == p.wl_stride)
      p.late_grid[k] = (int)std::min<size_t>(p.wl_stride, std::max<size_t>((size_t)2048, 2 * (size_t)h.wl_prev[k] + 256));
  }
  return p;
}

// ---- the entries that are not runs ----------------------------------------------------------------
// hc_derivatives_device, hc_histogram_device / hc_auto_thresholds_device, hc_edge_points_device, hc_gaussian_blur_device: their kernel parameters from views
// that passed check_view, complete but for the context's scratch (HistParams::hist, EdgePointsParams::items).  error: HC_E_ARG
// with this text, nothing may be allocated or launched.
struct DerivPlan { const char *error = nullptr; DerivParams dp{}; };
inline DerivPlan plan_derivatives(int W, int H, int C, const View &in, const View &dx, uintptr_t dy, int n, int ksize)
{
  DerivPlan P;
  DerivParams &d = P.dp;
  d.in = (const uint8_t *)in.p; d.in_pitch = in.pitch; d.in_frame_stride = in.fs;
  d.dx = (uint8_t *)dx.p; d.dy = (uint8_t *)dy; d.pitch = dx.pitch; d.frame_stride = dx.fs;  // (both planes: one pitch, one frame stride)
  d.W = W; d.H = H; d.nframes = n; d.channels = C; d.ksize = ksize;
  d.in_aligned = aligned4(in.p, in.pitch, in.fs);
  const uintptr_t oa = dx.p | dy | dx.pitch | dx.fs;
  d.out_align = (oa & 7u) == 0 ? 8 : (oa & 3u) == 0 ? 4 : 2;
  d.nstrips = deriv_strips(W); d.nchunks = deriv_chunks(H);
  const long long items = (long long)n * d.nstrips * d.nchunks;
  if (items > 0x7FFFFFF0ll) P.error = "too many work items (nframes x strips x row chunks)";
  else d.total_items = (int)items;
  return P;
}

// hc_gaussian_taps_q8: the Q8 taps of a ksize Gaussian as include/hipcanny.h states the rule.  false: ksize not 3 / 5 / 7, a
// sigma that is not finite, or taps that would break the contract of hc_gaussian_blur_device (nothing is written then)
inline bool gaussian_taps_q8(int ksize, double sigma, uint16_t *taps)
{
  if (!blur_ksize_ok(ksize) || !std::isfinite(sigma) || !taps) return false;
  static const uint16_t fixed[3][BLUR_MAX_TAPS] = { { 64, 128, 64 }, { 16, 64, 96, 64, 16 }, { 8, 28, 56, 72, 56, 28, 8 } };
  const int R = ksize / 2;
  if (sigma <= 0) {
    for (int i = 0; i < ksize; ++i) taps[i] = fixed[R - 1][i];
    return true;
  }
  double g[BLUR_MAX_TAPS], sum = 0;
  const double den = 2.0 * sigma * sigma;  // (0 for a sigma below 1e-154 or so: the centre tap alone, with no 0 / 0)
  for (int i = 0; i < ksize; ++i) { g[i] = i == R ? 1.0 : den > 0 ? std::exp(-(double)((i - R) * (i - R)) / den) : 0.0; sum += g[i]; }
  long t[BLUR_MAX_TAPS], rest = 0;
  double err = 0;
  for (int i = 0; i < R; ++i) {  // from the outside inwards, the rounding error carried to the next tap
    const double x = 256.0 * (g[i] / sum) + err, v = std::nearbyint(x);
    err = x - v;
    t[i] = t[ksize - 1 - i] = (long)v;
    rest += 2 * (long)v;
  }
  t[R] = 256 - rest;
  for (int i = 0; i < ksize; ++i)
    if (t[i] < 0 || t[i] > 256) return false;
  for (int i = 0; i < ksize; ++i) taps[i] = (uint16_t)t[i];
  return true;
}

static_assert(BLUR_REFLECT_101 == HC_BORDER_REFLECT_101 && BLUR_REPLICATE == HC_BORDER_REPLICATE, "canny_params.h names the header's borders");
// hc_gaussian_blur_device: everything the entry refuses but nframes > max_batch (check_views), and k_gauss8's parameters.  The
// views' byte ranges [p, p + (n - 1) fs + (H - 1) pitch + C W) must not overlap: the entry owns no scratch to stage through
struct BlurPlan { const char *error = nullptr; BlurParams bp{}; };
inline BlurPlan plan_gaussian_blur(int W, int H, int C, const View &in, const View &out, int n, int ksize, const uint16_t *taps, int border)
{
  BlurPlan P;
  BlurParams &b = P.bp;
  const size_t row = (size_t)C * W;
  if (!in.p || !out.p || !taps) return P.error = "null argument", P;
  if (!blur_ksize_ok(ksize)) return P.error = "ksize 3, 5 or 7", P;
  if (border != BLUR_REFLECT_101 && border != BLUR_REPLICATE) return P.error = "border must be HC_BORDER_REFLECT_101 or HC_BORDER_REPLICATE", P;
  unsigned sum = 0;
  for (int i = 0; i < ksize; ++i) {
    if (taps[i] > 256) return P.error = "a tap above 256 (Q8: 256 = 1.0)", P;
    sum += taps[i];
  }
  if (sum != 256) return P.error = "the taps must sum to 256 (Q8: 256 = 1.0)", P;
  if (n < 1) return P.error = "nframes out of range", P;
  for (const View *v : { &in, &out })
    if (const ViewFault f = check_view(*v, row, H, n, 1, true)) return P.error = VIEW_FAULT_TEXT[f], P;
  uintptr_t end[2];
  if (!view_end(in, row, H, n, &end[0]) || !view_end(out, row, H, n, &end[1])) return P.error = "a view wraps the address space", P;
  if (in.p < end[1] && out.p < end[0]) return P.error = "the input and output views overlap (in-place operation is not supported: blur into another buffer)", P;
  b.in = (const uint8_t *)in.p; b.in_pitch = in.pitch; b.in_frame_stride = in.fs;
  b.out = (uint8_t *)out.p; b.out_pitch = out.pitch; b.out_frame_stride = out.fs;
  b.W = W; b.H = H; b.nframes = n; b.channels = C; b.ksize = ksize; b.border = border;
  b.in_aligned = aligned4(in.p, in.pitch, in.fs); b.out_aligned = aligned4(out.p, out.pitch, out.fs);
  for (int i = 0; i < ksize; ++i) b.taps[i] = taps[i];
  b.nstrips = blur_strips(W); b.nchunks = blur_chunks(H);
  const long long items = (long long)n * b.nstrips * b.nchunks;
  if (items > 0x7FFFFFF0ll) P.error = "too many work items (nframes x strips x row chunks)";
  else b.total_items = (int)items;
  return P;
}

inline HistParams plan_histogram(int W, int H, int C, const View &in, int n)
{
  HistParams h{};
  h.in = (const uint8_t *)in.p; h.in_pitch = in.pitch; h.in_frame_stride = in.fs; h.row_bytes = W * C; h.H = H; h.nframes = n;
  h.chunk_rows = hist_chunk_rows(H, n); h.nchunks = (H + h.chunk_rows - 1) / h.chunk_rows;
  h.total_items = n * h.nchunks;  // (at most 1024 frames x 1024 chunks of 8 rows or more)
  return h;
}

// table_items: the context's table of per-item counts -- chunks have min(8, H) rows or more, so it holds any batch the context takes (3-channel contexts: three maps per frame, HC_OPT_PER_CHANNEL)
struct EdgePlan { const char *error = nullptr; EdgePointsParams ep{}; size_t table_items = 0; };
inline EdgePlan plan_edge_points(int W, int H, int C, int max_batch, const View &map, int n, uintptr_t counts, uintptr_t points, size_t capacity)
{
  EdgePlan P;
  EdgePointsParams &e = P.ep;
  e.map = (const uint8_t *)map.p; e.pitch = map.pitch; e.frame_stride = map.fs; e.counts = (u32 *)counts;
  e.points = (int32_t *)points; e.capacity = capacity; e.W = W; e.H = H; e.nframes = n;
  e.chunk_rows = hist_chunk_rows(H, n); e.nchunks = (H + e.chunk_rows - 1) / e.chunk_rows;
  const int min_rows = std::min(HIST_MIN_CHUNK_ROWS, H);
  P.table_items = (size_t)max_batch * (C == 3 ? 3 : 1) * (size_t)((H + min_rows - 1) / min_rows);
  const long long items = (long long)n * e.nchunks;
  if (capacity > SIZE_MAX / 8 / (size_t)n) P.error = "capacity * 8 * nframes overflows size_t";
  else if (items > 0x7FFFFFF0ll || P.table_items > 0x7FFFFFF0ull) P.error = "too many work items (nframes x row chunks)";
  else e.total_items = (int)items;
  return P;
}

// ---- hc_hough_lines_device / hc_hough_tables ------------------------------------------------------
// The geometry of cv::HoughLines' accumulator as include/hipcanny.h states it.  nullptr and both numbers, or the refusal's text
// and nothing written.  Every bound is tested on the doubles, before a conversion that could overflow.
constexpr double HOUGH_PI = 3.1415926535897932384626433832795;
inline const char *hough_geometry(int W, int H, double rho, double theta, double min_theta, double max_theta, int *numangle, int *numrho)
{
  if (W < 1 || H < 1) return "width and height must be positive";
  if (!std::isfinite(rho) || !(rho > 0) || !std::isfinite(theta) || !(theta > 0)) return "rho and theta must be finite and positive";
  if (!std::isfinite(min_theta) || !std::isfinite(max_theta) || max_theta < min_theta) return "min_theta and max_theta must be finite, min_theta <= max_theta";
  const double na = std::floor((max_theta - min_theta) / theta) + 1.0;
  const double nr = std::nearbyint((2.0 * ((double)W + (double)H) + 1.0) / rho);  // (half to even)
  if (!(nr >= 0) || (nr + 2.0) * 4.0 > (double)HOUGH_LDS_BYTES) return "an accumulator row, (numrho + 2) * 4 bytes, does not fit one workgroup's LDS (160 KiB): rho is too small for the frame";
  if (!(na >= 1) || !((na + 2.0) * (nr + 2.0) < 2147483648.0)) return "the accumulator, (numangle + 2) * (numrho + 2) cells, reaches 2^31 cells";
  int a = (int)na;
  if (a > 1 && std::fabs(HOUGH_PI - (double)(a - 1) * theta) < theta / 2) --a;
  *numangle = a;
  *numrho = (int)nr;
  return nullptr;
}

// The tables: irho and the running angle are floats, the trigonometry is libm's in double (include/hipcanny.h)
inline void hough_fill_tables(int numangle, double rho, double theta, double min_theta, float *tab_cos, float *tab_sin, float *tab_theta)
{
  const float irho = 1.0f / (float)rho;
  float ang = (float)min_theta;
  for (int n = 0; n < numangle; ++n) {
    tab_cos[n] = (float)(std::cos((double)ang) * (double)irho);
    tab_sin[n] = (float)(std::sin((double)ang) * (double)irho);
    tab_theta[n] = ang;
    ang += (float)theta;
  }
}

// hc_hough_tables: geometry and, with all three tables given, the tables.  Refusals write nothing.
inline const char *hough_tables(int W, int H, double rho, double theta, double min_theta, double max_theta, int *numangle, int *numrho, float *tab_cos,
                                float *tab_sin, float *tab_theta, size_t table_capacity)
{
  if (!numangle || !numrho) return "numangle and numrho must not be null";
  const bool tabs = tab_cos || tab_sin || tab_theta;
  if (tabs && (!tab_cos || !tab_sin || !tab_theta)) return "the three tables are given together or not at all";
  int a = 0, r = 0;
  if (const char *e = hough_geometry(W, H, rho, theta, min_theta, max_theta, &a, &r)) return e;
  if (tabs && table_capacity < (size_t)a) return "table_capacity is smaller than numangle";
  *numangle = a;
  *numrho = r;
  if (tabs) hough_fill_tables(a, rho, theta, min_theta, tab_cos, tab_sin, tab_theta);
  return nullptr;
}

// hc_hough_walk_tables: how hc_hough_segments_device walks a line of angle tab_theta[n] (include/hipcanny.h): the axis with one
// sample per step, and the sample m = rint(t * slope + line_rho * scale) on the other.  libm in double, as the tables above.
inline void hough_fill_walk_tables(int numangle, const float *tab_theta, int32_t *major, float *slope, float *scale)
{
  for (int n = 0; n < numangle; ++n) {
    const double a = (double)tab_theta[n], c = std::cos(a), s = std::sin(a);
    if (std::fabs(s) >= std::fabs(c)) { major[n] = 0; slope[n] = (float)(-c / s); scale[n] = (float)(1.0 / s); }
    else { major[n] = 1; slope[n] = (float)(-s / c); scale[n] = (float)(1.0 / c); }
  }
}

// Geometry and, with all three tables given, the walk tables; tab_theta (optional, numangle floats as hc_hough_tables gives them:
// the device entry uploads it beside the three) needs the tables too.  Refusals write nothing.
inline const char *hough_walk_tables(int W, int H, double rho, double theta, double min_theta, double max_theta, int *numangle, int32_t *major, float *slope,
                                     float *scale, size_t table_capacity, float *tab_theta = nullptr)
{
  if (!numangle) return "numangle must not be null";
  const bool tabs = major || slope || scale;
  if ((tabs || tab_theta) && (!major || !slope || !scale)) return "the three tables are given together or not at all";
  int a = 0, r = 0;
  if (const char *e = hough_geometry(W, H, rho, theta, min_theta, max_theta, &a, &r)) return e;
  if (tabs && table_capacity < (size_t)a) return "table_capacity is smaller than numangle";
  *numangle = a;
  if (!tabs) return nullptr;
  std::vector<float> tmp(3 * (size_t)a);  // the angles by the one rule that makes them (hough_fill_tables; cos and sin are not used)
  float *th = tab_theta ? tab_theta : tmp.data() + 2 * (size_t)a;
  hough_fill_tables(a, rho, theta, min_theta, tmp.data(), tmp.data() + a, th);
  hough_fill_walk_tables(a, th, major, slope, scale);
  return nullptr;
}

constexpr size_t HOUGH_MAX_PASS_FRAMES = 65535;  // frames of a pass at most: a frame is a row of k_hough_rank's grid (gridDim.y)
constexpr size_t HOUGH_SCRATCH_BYTES = (size_t)256 << 20;  // the context's bound by default (HC_OPT_TEST_HOUGH_SCRATCH sets another)
// Angles per workgroup of k_hough_vote.  More rows load every point less often, but a workgroup's LDS decides how many of them
// a CU holds, and the LDS atomics want waves to hide behind: measured at 1080p (24 KB rows, 30 frames, profiles/hough/README.md)
// two rows -- three workgroups per CU -- are fastest on sparse and on dense lists, one and three rows 7 - 10 % behind, four to six
// (two workgroups, then one) 25 - 50 % behind.  So: the rows that leave room for HOUGH_WGS_PER_CU workgroups, HOUGH_MAX_ROWS
// at most (rows much shorter than 1080p's have not been measured), and fewer while the pass has fewer workgroups than the chip
// has CUs.  hough_max_rows: what LDS, HOUGH_MAX_ROWS and numangle allow at all (HC_OPT_TEST_HOUGH_ROWS may force up to that).
constexpr int HOUGH_WGS_PER_CU = 3;
inline int hough_max_rows(int numangle, int numrho)
{
  const long long row = ((long long)numrho + 2) * 4;
  return (int)std::min<long long>(std::min<long long>(HOUGH_MAX_ROWS, HOUGH_LDS_BYTES / row), numangle);
}
inline int hough_rows_per_group(int numangle, int numrho, int frames)
{
  const long long row = ((long long)numrho + 2) * 4;
  int a = (int)std::min<long long>(hough_max_rows(numangle, numrho), std::max<long long>(1, HOUGH_LDS_BYTES / HOUGH_WGS_PER_CU / row));
  while (a > 1 && (long long)frames * ((numangle + a - 1) / a) < HOUGH_CUS) --a;
  return a;
}

// Everything hc_hough_lines_device refuses and decides, but for the context pointer.  hp describes the FIRST pass with the
// scratch and table pointers null; hough_pass gives pass k with them patched in.  A refused plan holds nothing but its text.
struct HoughPlan {
  const char *error = nullptr;
  HoughParams hp{};
  int frames = 0, frames_per_pass = 0, passes = 0;
  size_t frame_peaks_bytes = 0, frame_accum_bytes = 0, frame_items_bytes = 0;  // scratch per frame
  size_t scratch_bytes = 0;   // frames_per_pass * the three: [peaks | accumulators | items]
  long long total_work = 0;   // workgroups of k_hough_vote over all passes: frames x groups
  unsigned vote_grid = 0, rows_grid = 0, scan_grid = 0, rank_grid_x = 0, rank_grid_y = 0;  // of a full pass (rank: 0 when line_capacity == 0 or no cell can be a peak)
};
inline HoughPlan plan_hough_lines(int W, int H, int max_frames, uintptr_t points, uintptr_t point_counts, size_t point_capacity, int n, double rho,
                                  double theta, int threshold, double min_theta, double max_theta, uintptr_t line_counts, uintptr_t lines,
                                  size_t line_capacity, size_t scratch_bound, int rows_forced = 0)
{
  HoughPlan P;
  auto refuse = [](const char *text) { HoughPlan R; R.error = text; return R; };
  if (!points || !point_counts || !line_counts) return refuse("null argument");
  if (line_capacity && !lines) return refuse("d_lines is null with line_capacity > 0");
  if (points & 7u) return refuse("d_points must be 8-byte aligned");
  if ((point_counts | line_counts | lines) & 3u) return refuse("d_point_counts, d_line_counts and d_lines must be 4-byte aligned");
  if (n < 1 || n > max_frames) return refuse("nframes out of range");
  if (threshold < 0) return refuse("threshold must not be negative");
  int numangle = 0, numrho = 0;
  if (const char *e = hough_geometry(W, H, rho, theta, min_theta, max_theta, &numangle, &numrho)) return refuse(e);
  if (point_capacity > SIZE_MAX / 8 / (size_t)n) return refuse("point_capacity * 8 * nframes overflows size_t");
  if (line_capacity > SIZE_MAX / 12 / (size_t)n) return refuse("line_capacity * 12 * nframes overflows size_t");
  const size_t cells = (size_t)(numangle + 2) * (size_t)(numrho + 2), peak_cap = (size_t)numangle * (size_t)((numrho + 1) / 2);
  P.frame_peaks_bytes = peak_cap * 8; P.frame_accum_bytes = cells * 4; P.frame_items_bytes = (size_t)numangle * 4;
  const size_t per_frame = P.frame_peaks_bytes + P.frame_accum_bytes + P.frame_items_bytes;  // (below 2^31 * 8 + 2^33 + 2^33)
  if (scratch_bound < per_frame) return refuse("one frame's accumulator and peak list exceed the context's scratch bound (256 MiB): a coarser rho or theta");
  P.frames = n;
  P.frames_per_pass = (int)std::min<size_t>(std::min<size_t>((size_t)n, scratch_bound / per_frame), HOUGH_MAX_PASS_FRAMES);
  P.passes = (n + P.frames_per_pass - 1) / P.frames_per_pass;
  P.scratch_bytes = (size_t)P.frames_per_pass * per_frame;
  if ((long long)P.frames_per_pass * numangle > 0x7FFFFFF0ll) return refuse("too many work items (frames of a pass x numangle)");
  HoughParams &h = P.hp;
  h.points = (const int32_t *)points; h.point_counts = (const u32 *)point_counts; h.point_capacity = point_capacity;
  h.line_counts = (u32 *)line_counts; h.lines = (float *)lines; h.line_capacity = line_capacity; h.peak_cap = peak_cap;
  h.numangle = numangle; h.numrho = numrho; h.nframes = P.frames_per_pass; h.threshold = threshold; h.rho = (float)rho;
  // rows_forced > 0 (HC_OPT_TEST_HOUGH_ROWS: measurements): that many rows where LDS, HOUGH_MAX_ROWS and numangle allow it
  h.rows = rows_forced > 0 ? std::min(rows_forced, hough_max_rows(numangle, numrho)) : hough_rows_per_group(numangle, numrho, P.frames_per_pass);
  h.groups = (numangle + h.rows - 1) / h.rows;
  P.total_work = (long long)n * h.groups;
  P.vote_grid = (unsigned)(P.frames_per_pass * h.groups);  // (at most frames x numangle)
  P.rows_grid = (unsigned)(((long long)P.frames_per_pass * numangle + 3) / 4);
  P.scan_grid = (unsigned)((P.frames_per_pass + 3) / 4);
  if (line_capacity && peak_cap) { P.rank_grid_x = (unsigned)((peak_cap + HOUGH_RANK_THREADS - 1) / HOUGH_RANK_THREADS); P.rank_grid_y = (unsigned)P.frames_per_pass; }
  return P;
}

// Pass k of a plan that was not refused (0 <= k < passes), on `scratch` (scratch_bytes, 8-byte aligned) and the context's tables
// [3][numangle] = cos, sin, theta
inline HoughParams hough_pass(const HoughPlan &P, int k, uintptr_t scratch, uintptr_t tables)
{
  HoughParams h = P.hp;
  const int f0 = k * P.frames_per_pass;
  h.nframes = std::min(P.frames_per_pass, P.frames - f0);
  h.points += (size_t)f0 * h.point_capacity * 2;
  h.point_counts += f0;
  h.line_counts += f0;
  if (h.lines) h.lines += (size_t)f0 * h.line_capacity * 3;
  h.peaks = (u32 *)scratch;
  h.accum = (int32_t *)(scratch + (size_t)P.frames_per_pass * P.frame_peaks_bytes);
  h.items = (u32 *)(scratch + (size_t)P.frames_per_pass * (P.frame_peaks_bytes + P.frame_accum_bytes));
  h.tab_cos = (const float *)tables;
  h.tab_sin = h.tab_cos + h.numangle;
  h.tab_theta = h.tab_sin + h.numangle;
  return h;
}

// ---- hc_hough_segments_device ---------------------------------------------------------------------
// Everything the entry refuses and decides, but for the context pointer: sp is complete but for the context's scratch (items,
// the four tables: seg_on_scratch patches them in).  A refused plan holds nothing but its text.
struct SegPlan {
  const char *error = nullptr;
  SegParams sp{};
  size_t items_bytes = 0;   // scratch [nframes][line_capacity] u32
  size_t table_bytes = 0;   // scratch [4][numangle] 4-byte words: theta, major, slope, scale
  unsigned lines_grid = 0, scan_grid = 0;  // workgroups of four waves: k_seg_count / k_seg_emit (a wave per line slot); k_seg_scan (a wave per frame)
  bool emit = false;        // k_seg_emit is launched (seg_capacity > 0)
};
inline SegPlan plan_hough_segments(int W, int H, int max_frames, const View &map, uintptr_t lines, uintptr_t line_counts, size_t line_capacity, int n, double rho,
                                   double theta, double min_theta, double max_theta, int min_length, int max_gap, uintptr_t seg_counts, uintptr_t segs,
                                   size_t seg_capacity)
{
  SegPlan P;
  auto refuse = [](const char *text) { SegPlan R; R.error = text; return R; };
  if (!map.p || !lines || !line_counts || !seg_counts) return refuse("null argument");
  if (seg_capacity && !segs) return refuse("d_segs is null with seg_capacity > 0");
  if ((lines | line_counts | seg_counts) & 3u) return refuse("d_lines, d_line_counts and d_seg_counts must be 4-byte aligned");
  if (segs & 15u) return refuse("d_segs must be 16-byte aligned");
  if (min_length < 0 || max_gap < 0) return refuse("min_length and max_gap must not be negative");
  if (n < 1 || n > max_frames) return refuse("nframes out of range");
  int numangle = 0, numrho = 0;
  if (const char *e = hough_geometry(W, H, rho, theta, min_theta, max_theta, &numangle, &numrho)) return refuse(e);
  if (const ViewFault f = check_view(map, (size_t)W, H, n, 1, true)) return refuse(VIEW_FAULT_TEXT[f]);
  if (!line_capacity) return refuse("line_capacity must be positive");
  if (line_capacity > SIZE_MAX / 12 / (size_t)n) return refuse("line_capacity * 12 * nframes overflows size_t");
  if (seg_capacity > SIZE_MAX / 16 / (size_t)n) return refuse("seg_capacity * 16 * nframes overflows size_t");
  if (line_capacity > (size_t)0x7FFFFFF0 / (size_t)n) return refuse("too many work items (nframes x line_capacity)");
  // a walk of L steps holds at most ceil(L / 2) segments: a frame's count stays below 2^32
  if (line_capacity > (size_t)0xFFFFFFFFu / (((size_t)std::max(W, H) + 1) / 2)) return refuse("line_capacity * ceil(max(width, height) / 2) reaches 2^32: a frame's segment count would not fit uint32");
  SegParams &s = P.sp;
  s.map = (const uint8_t *)map.p; s.pitch = map.pitch; s.frame_stride = map.fs;
  s.lines = (const float *)lines; s.line_counts = (const u32 *)line_counts; s.line_capacity = line_capacity;
  s.seg_counts = (u32 *)seg_counts; s.segs = (int32_t *)segs; s.seg_capacity = seg_capacity;
  s.W = W; s.H = H; s.nframes = n; s.numangle = numangle; s.min_length = min_length; s.max_gap = max_gap;
  s.total_items = (int)((size_t)n * line_capacity);
  P.items_bytes = (size_t)s.total_items * 4;
  P.table_bytes = (size_t)numangle * 16;
  P.lines_grid = (unsigned)(((long long)s.total_items + 3) / 4);
  P.scan_grid = (unsigned)((n + 3) / 4);
  P.emit = seg_capacity > 0;
  return P;
}

// The parameters of a plan that was not refused, on the context's scratch: `items` (items_bytes) and `tables` (table_bytes)
inline SegParams seg_on_scratch(const SegPlan &P, uintptr_t items, uintptr_t tables)
{
  SegParams s = P.sp;
  s.items = (u32 *)items;
  s.tab_theta = (const float *)tables;
  s.tab_major = (const int32_t *)(tables + (size_t)s.numangle * 4);
  s.tab_slope = (const float *)(tables + (size_t)s.numangle * 8);
  s.tab_scale = (const float *)(tables + (size_t)s.numangle * 12);
  return s;
}

// ---- hc_hough_circles_device / hc_hough_circle_geometry -------------------------------------------
// The accumulator of the centre votes and the smallest squared distance of two kept centres, as include/hipcanny.h states them.
// nullptr and the three numbers, or the refusal's text and nothing written.
constexpr int CIRCLE_COORD_LIMIT = 1 << 20;  // width + max_radius and height + max_radius stay below: the Q10 walk stays inside int32
inline const char *hough_circle_geometry(int W, int H, double dp, double min_dist, int min_radius, int max_radius, int *acc_width, int *acc_height,
                                         long long *min_d2)
{
  if (!acc_width || !acc_height || !min_d2) return "acc_width, acc_height and min_d2 must not be null";
  if (W < 1 || H < 1) return "width and height must be positive";
  if (!std::isfinite(dp) || !(dp >= 1)) return "dp must be finite and at least 1";
  if (!std::isfinite(min_dist) || min_dist < 0) return "min_dist must be finite and not negative";
  if (min_radius < 1 || max_radius < min_radius) return "1 <= min_radius <= max_radius is required";
  if ((long long)max_radius - min_radius + 3 > CIRCLE_MAX_HIST) return "a radius histogram, max_radius - min_radius + 3 words, exceeds 4096 words";
  if ((long long)W + max_radius >= CIRCLE_COORD_LIMIT || (long long)H + max_radius >= CIRCLE_COORD_LIMIT) return "width + max_radius and height + max_radius must stay below 2^20";
  const float idp = 1.0f / (float)dp;
  const double aw = std::ceil((double)((float)W * idp)), ah = std::ceil((double)((float)H * idp));  // (at most 2^20: dp >= 1)
  if (!(aw >= 1) || !(ah >= 1)) return "dp is so large that the accumulator has no cell";  // ((float)dp infinite, or a product that underflows)
  if (!((aw + 2.0) * (ah + 2.0) < 2147483648.0)) return "the accumulator, (acc_height + 2) * (acc_width + 2) cells, reaches 2^31 cells";
  const double md = min_dist / dp, v = md * md;  // (no two cells lie 2^62 apart: a larger bound is that one)
  *acc_width = (int)aw;
  *acc_height = (int)ah;
  *min_d2 = v >= 4611686018427387904.0 ? (1ll << 62) : (long long)std::ceil(v);
  return nullptr;
}

// Everything hc_hough_circles_device refuses and decides, but for the context pointer.  cp describes the FIRST pass with the
// scratch pointers null; circle_pass gives pass k with them patched in.  A refused plan holds nothing but its text.
struct CirclePlan {
  const char *error = nullptr;
  CircleParams cp{};
  int frames = 0, frames_per_pass = 0, passes = 0;
  // scratch per frame, in the order of the scratch's sections (each section holds frames_per_pass frames)
  size_t frame_ranked_bytes = 0, frame_kept_bytes = 0, frame_peaks_bytes = 0, frame_accum_bytes = 0, frame_rows_bytes = 0, frame_items_bytes = 0, frame_counts_bytes = 0;
  size_t scratch_bytes = 0;
  // The grids: cp.vote_groups and cp.rank_groups are the workgroups per frame of k_circle_vote and k_circle_rank, and the launch
  // reads them there.  Every other grid is one of cp.nframes, cp.centre_capacity and what launch_hough_peaks derives for its own
  // kernels (hough_circles.hip, hough.hip): the plan keeps no second copy of them.
  bool emit = false;  // k_circle_radii<true> is launched (circle_capacity > 0)
};
inline CirclePlan plan_hough_circles(int W, int H, int max_frames, uintptr_t points, uintptr_t point_counts, size_t point_capacity, const View &dx, uintptr_t dy,
                                     int n, double dp, double min_dist, int votes_threshold, int min_radius, int max_radius, size_t centre_capacity,
                                     uintptr_t circle_counts, uintptr_t circles, size_t circle_capacity, size_t scratch_bound)
{
  CirclePlan P;
  auto refuse = [](const char *text) { CirclePlan R; R.error = text; return R; };
  if (!points || !point_counts || !dx.p || !dy || !circle_counts) return refuse("null argument");
  if (circle_capacity && !circles) return refuse("d_circles is null with circle_capacity > 0");
  if (points & 7u) return refuse("d_points must be 8-byte aligned");
  if ((point_counts | circle_counts) & 3u) return refuse("d_point_counts and d_circle_counts must be 4-byte aligned");
  if (circles & 15u) return refuse("d_circles must be 16-byte aligned");
  if (n < 1 || n > max_frames) return refuse("nframes out of range");
  if (votes_threshold < 0) return refuse("votes_threshold must not be negative");
  if (centre_capacity < 1 || centre_capacity > (size_t)CIRCLE_MAX_CENTRES) return refuse("centre_capacity must lie in 1 .. 4096");
  int AW = 0, AH = 0;
  long long min_d2 = 0;
  if (const char *e = hough_circle_geometry(W, H, dp, min_dist, min_radius, max_radius, &AW, &AH, &min_d2)) return refuse(e);
  const View dyv{ dy, dx.pitch, dx.fs };
  if (const ViewFault f = check_view(dx, 2 * (size_t)W, H, n, 2, true)) return refuse(VIEW_FAULT_TEXT[f]);
  if (const ViewFault f = check_view(dyv, 2 * (size_t)W, H, n, 2, true)) return refuse(VIEW_FAULT_TEXT[f]);
  uintptr_t end = 0;
  if (!view_end(dx, 2 * (size_t)W, H, n, &end) || !view_end(dyv, 2 * (size_t)W, H, n, &end)) return refuse("a view wraps the address space");
  if (point_capacity > SIZE_MAX / 8 / (size_t)n) return refuse("point_capacity * 8 * nframes overflows size_t");
  if (circle_capacity > SIZE_MAX / 16 / (size_t)n) return refuse("circle_capacity * 16 * nframes overflows size_t");
  const size_t cells = (size_t)(AH + 2) * (size_t)(AW + 2), peak_cap = (size_t)AH * (size_t)((AW + 1) / 2);
  P.frame_ranked_bytes = P.frame_kept_bytes = centre_capacity * 16;
  P.frame_peaks_bytes = peak_cap * 8; P.frame_accum_bytes = cells * 4; P.frame_rows_bytes = (size_t)AH * 4;
  P.frame_items_bytes = centre_capacity * 4; P.frame_counts_bytes = 8;
  const size_t per_frame = P.frame_ranked_bytes + P.frame_kept_bytes + P.frame_peaks_bytes + P.frame_accum_bytes + P.frame_rows_bytes + P.frame_items_bytes
                           + P.frame_counts_bytes;  // (below 2^33 + 2^33 + a few 2^17)
  if (scratch_bound < per_frame) return refuse("one frame's accumulator, peak list and centre lists exceed the context's scratch bound: use a larger dp");
  P.frames = n;
  P.frames_per_pass = (int)std::min<size_t>(std::min<size_t>((size_t)n, scratch_bound / per_frame), HOUGH_MAX_PASS_FRAMES);
  P.passes = (n + P.frames_per_pass - 1) / P.frames_per_pass;
  P.scratch_bytes = (size_t)P.frames_per_pass * per_frame;
  if ((long long)P.frames_per_pass * AH > 0x7FFFFFF0ll) return refuse("too many work items (frames of a pass x accumulator rows)");
  CircleParams &c = P.cp;
  c.points = (const int32_t *)points; c.point_counts = (const u32 *)point_counts; c.point_capacity = point_capacity;
  c.dx = (const int16_t *)dx.p; c.dy = (const int16_t *)dy; c.pitch = dx.pitch; c.frame_stride = dx.fs;
  c.circle_counts = (u32 *)circle_counts; c.circles = (float *)circles; c.circle_capacity = circle_capacity; c.peak_cap = peak_cap;
  c.min_d2 = min_d2; c.W = W; c.H = H; c.AW = AW; c.AH = AH; c.nframes = P.frames_per_pass; c.centre_capacity = (int)centre_capacity;
  c.threshold = votes_threshold; c.min_radius = min_radius; c.max_radius = max_radius; c.idp = 1.0f / (float)dp; c.dp = (float)dp;
  c.vote_groups = (unsigned)std::min<size_t>(std::max<size_t>((point_capacity + CIRCLE_THREADS - 1) / CIRCLE_THREADS, 1), CIRCLE_VOTE_GROUPS);
  c.rank_groups = (unsigned)((peak_cap + HOUGH_RANK_THREADS - 1) / HOUGH_RANK_THREADS);  // (at least 1: AW, AH >= 1; below 2^22: fewer than 2^30 peaks)
  P.emit = circle_capacity > 0;
  return P;
}

// Pass k of a plan that was not refused (0 <= k < passes), on `scratch` (scratch_bytes, 16-byte aligned): the sections lie in the
// order ranked | kept | peaks | accumulators | per-row counts | per-centre counts | npeaks | nkept, the widest alignment first
inline CircleParams circle_pass(const CirclePlan &P, int k, uintptr_t scratch)
{
  CircleParams c = P.cp;
  const int f0 = k * P.frames_per_pass;
  const size_t fpp = (size_t)P.frames_per_pass;
  c.nframes = std::min(P.frames_per_pass, P.frames - f0);
  c.points += (size_t)f0 * c.point_capacity * 2;
  c.point_counts += f0;
  c.dx = (const int16_t *)((uintptr_t)c.dx + (size_t)f0 * c.frame_stride);
  c.dy = (const int16_t *)((uintptr_t)c.dy + (size_t)f0 * c.frame_stride);
  c.circle_counts += f0;
  if (c.circles) c.circles += (size_t)f0 * c.circle_capacity * 4;
  uintptr_t q = scratch;
  c.ranked = (int32_t *)q; q += fpp * P.frame_ranked_bytes;
  c.kept = (int32_t *)q;   q += fpp * P.frame_kept_bytes;
  c.peaks = (u32 *)q;      q += fpp * P.frame_peaks_bytes;
  c.accum = (int32_t *)q;  q += fpp * P.frame_accum_bytes;
  c.row_items = (u32 *)q;  q += fpp * P.frame_rows_bytes;
  c.items = (u32 *)q;      q += fpp * P.frame_items_bytes;
  c.npeaks = (u32 *)q;     q += fpp * 4;
  c.nkept = (u32 *)q;
  return c;
}

// ---- hc_connected_components_device ---------------------------------------------------------------
// Everything the entry refuses and decides, but for the context pointer.  cp describes the FIRST pass with the table pointer
// null; ccl_pass gives pass k with it patched in.  A refused plan holds nothing but its text.  The scratch is the table of
// per-chunk root counts alone ([frames_per_pass][nchunks] words: it grows with the frame's height, so it falls under the
// context's scratch bound and a batch is cut into passes of as many frames as fit); the sums of the statistics live in the
// caller's own rows until the last kernel turns them into the result.
struct CclPlan {
  const char *error = nullptr;
  CclParams cp{};
  int frames = 0, frames_per_pass = 0, passes = 0;
  size_t frame_items_bytes = 0, scratch_bytes = 0;
  bool stats = false;  // k_ccl_rows, k_ccl_stats and k_ccl_finish are launched (capacity > 0)
};
inline CclPlan plan_connected_components(int W, int H, int max_frames, const View &map, const View &labels, int n, int connectivity, uintptr_t counts,
                                         uintptr_t stats, uintptr_t centroids, size_t capacity, size_t scratch_bound)
{
  CclPlan P;
  auto refuse = [](const char *text) { CclPlan R; R.error = text; return R; };
  if (!map.p || !labels.p || !counts) return refuse("null argument");
  if (capacity && (!stats || !centroids)) return refuse("d_stats or d_centroids is null with capacity > 0");
  if (connectivity != 4 && connectivity != 8) return refuse("connectivity must be 4 or 8");
  if ((counts | stats) & 3u) return refuse("d_counts and d_stats must be 4-byte aligned");
  if (centroids & 7u) return refuse("d_centroids must be 8-byte aligned");
  if (n < 1 || n > max_frames) return refuse("nframes out of range");
  if (W < 1 || H < 1) return refuse("width and height must be positive");
  if ((long long)W * H >= 0x7FFFFFFFll) return refuse("width * height reaches 2^31 - 1 pixels");
  if (const ViewFault f = check_view(map, (size_t)W, H, n, 1, true)) return refuse(VIEW_FAULT_TEXT[f]);
  if (const ViewFault f = check_view(labels, 4 * (size_t)W, H, n, 4, true))
    return refuse(f == VIEW_ALIGN ? "d_labels, label_pitch and label_frame_stride must be multiples of 4" : f == VIEW_PITCH ? "label_pitch smaller than a row of int32 labels" : VIEW_FAULT_TEXT[f]);
  uintptr_t end[2];
  if (!view_end(map, (size_t)W, H, n, &end[0]) || !view_end(labels, 4 * (size_t)W, H, n, &end[1])) return refuse("a view wraps the address space");
  if (map.p < end[1] && labels.p < end[0]) return refuse("the map and the label plane overlap");
  if (capacity > SIZE_MAX / 20 / (size_t)n) return refuse("capacity * 20 * nframes overflows size_t");
  if (capacity > SIZE_MAX / 16 / (size_t)n) return refuse("capacity * 16 * nframes overflows size_t");
  CclParams &c = P.cp;
  c.chunk_rows = hist_chunk_rows(H, n); c.nchunks = (H + c.chunk_rows - 1) / c.chunk_rows;
  P.frame_items_bytes = 4 * (size_t)c.nchunks;
  if (scratch_bound < P.frame_items_bytes) return refuse("one frame's table of per-chunk counts exceeds the context's scratch bound");
  P.frames = n;
  P.frames_per_pass = (int)std::min<size_t>(std::min<size_t>((size_t)n, scratch_bound / P.frame_items_bytes), HOUGH_MAX_PASS_FRAMES);
  P.passes = (n + P.frames_per_pass - 1) / P.frames_per_pass;
  P.scratch_bytes = (size_t)P.frames_per_pass * P.frame_items_bytes;
  c.tiles_x = (W + CCL_TILE_W - 1) / CCL_TILE_W; c.tiles_y = (H + CCL_TILE_H - 1) / CCL_TILE_H;
  const long long tiles = (long long)c.tiles_x * c.tiles_y, border = (long long)(c.tiles_y - 1) * W + (long long)(c.tiles_x - 1) * H;
  if (tiles > (1ll << 23) || border > 0x7FFFFFF0ll || (long long)P.frames_per_pass * c.nchunks > 0x7FFFFFF0ll)
    return refuse("too many work items (tiles, border pixels or frames of a pass x row chunks)");
  c.map = (const uint8_t *)map.p; c.pitch = map.pitch; c.frame_stride = map.fs;
  c.labels = (int32_t *)labels.p; c.label_pitch = labels.pitch; c.label_frame_stride = labels.fs;
  c.counts = (u32 *)counts; c.stats = (int32_t *)stats; c.sums = (unsigned long long *)centroids; c.capacity = capacity;
  c.W = W; c.H = H; c.nframes = P.frames_per_pass; c.connectivity = connectivity;
  c.border_items = (unsigned)border; c.total_items = c.nframes * c.nchunks;
  const size_t rows = std::min<size_t>(capacity, (size_t)W * (size_t)H + 1);  // (no frame has more components than pixels)
  c.row_groups = (unsigned)std::min<size_t>((rows + CCL_THREADS - 1) / CCL_THREADS, CCL_ROW_GROUPS);
  P.stats = capacity > 0;
  return P;
}

// Pass k of a plan that was not refused (0 <= k < passes), on the table `items` (scratch_bytes, 4-byte aligned)
inline CclParams ccl_pass(const CclPlan &P, int k, uintptr_t items)
{
  CclParams c = P.cp;
  const int f0 = k * P.frames_per_pass;
  c.nframes = std::min(P.frames_per_pass, P.frames - f0);
  c.total_items = c.nframes * c.nchunks;
  c.map += (size_t)f0 * c.frame_stride;
  c.labels = (int32_t *)((uintptr_t)c.labels + (size_t)f0 * c.label_frame_stride);
  c.counts += f0;
  if (c.capacity) { c.stats += (size_t)f0 * c.capacity * 5; c.sums += (size_t)f0 * c.capacity * 2; }
  c.items = (u32 *)items;
  return c;
}

// ---- hc_morphology_device -------------------------------------------------------------------------
static_assert(MORPH_ERODE == HC_MORPH_ERODE && MORPH_DILATE == HC_MORPH_DILATE && MORPH_OPEN == HC_MORPH_OPEN && MORPH_CLOSE == HC_MORPH_CLOSE
              && MORPH_GRADIENT == HC_MORPH_GRADIENT, "canny_params.h names the header's operations");
// hc_structuring_element: the half-widths of cv::getStructuringElement's three shapes as include/hipcanny.h states the rule.
// false: a shape outside the enum, ksize not 3 / 5 / 7 or spans null (nothing is written then)
inline bool structuring_spans(int shape, int ksize, int8_t *spans)
{
  if (!blur_ksize_ok(ksize) || !spans || (shape != HC_MORPH_RECT && shape != HC_MORPH_CROSS && shape != HC_MORPH_ELLIPSE)) return false;
  const int r = ksize / 2;
  for (int j = 0; j < ksize; ++j) {
    const double dy = (double)(j - r);
    spans[j] = shape == HC_MORPH_RECT ? (int8_t)r : shape == HC_MORPH_CROSS ? (int8_t)(j == r ? r : 0)
                                      : (int8_t)std::nearbyint((double)r * std::sqrt(((double)(r * r) - dy * dy) / (double)(r * r)));
  }
  return true;
}

// Everything the entry refuses and decides, but for the context pointer.  A call is one or two launches of k_morph8 per pass:
// ERODE / DILATE one; GRADIENT two with no scratch (dilate into the output, then erode subtracted from it in place); OPEN / CLOSE
// two through the context's scratch, which holds the intermediate frames of one pass as tight u8 frames of scratch_pitch =
// channels * W rounded up to a multiple of 4 bytes per row (so that the 256-byte aligned scratch always takes the dword path), H
// rows per frame with no gap between the frames.  The scratch falls under the context's scratch bound: a batch is cut into passes
// of as many whole frames as fit.  mp describes the FIRST launch of the first pass as if it went from the input to the output
// view; morph_pass gives the launches of pass k.  A refused plan holds nothing but its text.
struct MorphPlan {
  const char *error = nullptr;
  MorphParams mp{};
  int op = 0, stages = 0;  // launches per pass
  int frames = 0, frames_per_pass = 0, passes = 0;
  size_t scratch_pitch = 0, scratch_frame_bytes = 0, scratch_bytes = 0;  // 0: the operation needs none
};
inline MorphPlan plan_morphology(int W, int H, int ctxC, bool per_channel, int max_batch, const View &in, const View &out, int n, int channels, int op, int ksize,
                                 const int8_t *spans, size_t scratch_bound)
{
  MorphPlan P;
  auto refuse = [](const char *text) { MorphPlan R; R.error = text; return R; };
  if (!in.p || !out.p || !spans) return refuse("null argument");
  if (channels != 1 && channels != 3) return refuse("channels must be 1 or 3");
  if (channels == 3 && ctxC != 3) return refuse("channels = 3 needs a 3-channel context");
  if (op != MORPH_ERODE && op != MORPH_DILATE && op != MORPH_OPEN && op != MORPH_CLOSE && op != MORPH_GRADIENT) return refuse("op must be one of HC_MORPH_ERODE .. HC_MORPH_GRADIENT");
  if (!blur_ksize_ok(ksize)) return refuse("ksize 3, 5 or 7");
  bool any = false;
  for (int j = 0; j < ksize; ++j) {
    if (spans[j] < -1 || spans[j] > ksize / 2) return refuse("a span outside -1 .. ksize / 2");
    any = any || spans[j] >= 0;
  }
  if (!any) return refuse("every row of the element is empty");
  if (W < 1 || H < 1) return refuse("width and height must be positive");
  const int max_frames = channels == 1 ? max_batch * (per_channel ? 3 : 1) : max_batch;
  if (n < 1 || n > max_frames) return refuse("nframes out of range");
  const size_t row = (size_t)channels * W;
  for (const View *v : { &in, &out })
    if (const ViewFault f = check_view(*v, row, H, n, 1, true)) return refuse(VIEW_FAULT_TEXT[f]);
  uintptr_t end[2];
  if (!view_end(in, row, H, n, &end[0]) || !view_end(out, row, H, n, &end[1])) return refuse("a view wraps the address space");
  if (in.p < end[1] && out.p < end[0]) return refuse("the input and output views overlap (in-place operation is not supported)");
  MorphParams &m = P.mp;
  m.nstrips = blur_strips(W); m.nchunks = blur_chunks(H);
  P.op = op; P.frames = n; P.frames_per_pass = n; P.passes = 1;
  P.stages = op == MORPH_ERODE || op == MORPH_DILATE ? 1 : 2;
  if (op == MORPH_OPEN || op == MORPH_CLOSE) {
    P.scratch_pitch = round_up(row, 4);
    if (reaches_4g(H, P.scratch_pitch)) return refuse(VIEW_FAULT_TEXT[VIEW_4G]);
    P.scratch_frame_bytes = (size_t)H * P.scratch_pitch;
    if (scratch_bound < P.scratch_frame_bytes) return refuse("one frame of intermediate results exceeds the context's scratch bound");
    P.frames_per_pass = (int)std::min<size_t>((size_t)n, scratch_bound / P.scratch_frame_bytes);
    P.passes = (n + P.frames_per_pass - 1) / P.frames_per_pass;
    P.scratch_bytes = (size_t)P.frames_per_pass * P.scratch_frame_bytes;
  }
  if ((long long)P.frames_per_pass * m.nstrips * m.nchunks > 0x7FFFFFF0ll) return refuse("too many work items (frames of a pass x strips x row chunks)");
  m.in = (const uint8_t *)in.p; m.in_pitch = in.pitch; m.in_frame_stride = in.fs;
  m.out = (uint8_t *)out.p; m.out_pitch = out.pitch; m.out_frame_stride = out.fs;
  m.W = W; m.H = H; m.nframes = P.frames_per_pass; m.channels = channels; m.ksize = ksize;
  m.in_aligned = aligned4(in.p, in.pitch, in.fs); m.out_aligned = aligned4(out.p, out.pitch, out.fs);
  m.total_items = m.nframes * m.nstrips * m.nchunks;
  // the levels: the distinct half-widths, ascending
  for (int a = 0; a <= ksize / 2; ++a) {
    bool used = false;
    for (int j = 0; j < ksize; ++j) used = used || spans[j] == a;
    if (used) m.level[m.nlevels++] = (int8_t)a;
  }
  for (int j = 0; j <= MORPH_MAX_K; ++j) {
    m.row_level[j] = -1;
    for (int l = 0; j < ksize && l < m.nlevels; ++l)
      if (spans[j] == m.level[l]) m.row_level[j] = (int8_t)l;
  }
  return P;
}

// The launches of pass k of a plan that was not refused (0 <= k < passes), in order; scratch: scratch_bytes, 4-byte aligned (not
// read when the plan needs none)
struct MorphPass { int stages = 0; MorphParams st[2]; };
inline MorphPass morph_pass(const MorphPlan &P, int k, uintptr_t scratch)
{
  MorphPass R;
  R.stages = P.stages;
  const int f0 = k * P.frames_per_pass;
  MorphParams m = P.mp;
  m.nframes = std::min(P.frames_per_pass, P.frames - f0);
  m.total_items = m.nframes * m.nstrips * m.nchunks;
  m.in += (size_t)f0 * m.in_frame_stride;
  m.out += (size_t)f0 * m.out_frame_stride;
  R.st[0] = R.st[1] = m;
  MorphParams &a = R.st[0], &b = R.st[1];
  switch (P.op) {
  case MORPH_ERODE: a.complement = 1; break;
  case MORPH_DILATE: break;
  case MORPH_GRADIENT: b.complement = 1; b.subtract = 1; break;  // dilate into the output, then out -= erode
  default:  // OPEN: erode then dilate; CLOSE: dilate then erode -- through the scratch
    a.complement = P.op == MORPH_OPEN; b.complement = P.op == MORPH_CLOSE;
    a.out = (uint8_t *)scratch; a.out_pitch = P.scratch_pitch; a.out_frame_stride = P.scratch_frame_bytes; a.out_aligned = 1;
    b.in = (const uint8_t *)scratch; b.in_pitch = P.scratch_pitch; b.in_frame_stride = P.scratch_frame_bytes; b.in_aligned = 1;
    break;
  }
  return R;
}

// ---- hc_distance_transform_device -----------------------------------------------------------------
static_assert(DT_TO_NONZERO == HC_DT_TO_NONZERO && DT_TO_ZERO == HC_DT_TO_ZERO && DT_SQUARED_I32 == HC_DT_SQUARED_I32 && DT_F32 == HC_DT_F32 && DT_NONE == HC_DT_NONE,
              "canny_params.h names the header's targets, types and HC_DT_NONE");
// Everything the entry refuses and decides, but for the context pointer.  dp is the parameter block of both kernels (k_dt_cols
// on a grid of col_groups x nframes workgroups, k_dt_rows on row_groups x nframes with lds_bytes of LDS); there is no scratch and
// there are no passes.  nearest.p == 0: the call wants no nearest plane (its pitch and stride are not looked at then).  A refused
// plan holds nothing but its text.
struct DistPlan { const char *error = nullptr; DistParams dp{}; };
inline DistPlan plan_distance_transform(int W, int H, int max_frames, const View &map, const View &dist, const View &nearest, int n, int target, int dist_type)
{
  DistPlan P;
  auto refuse = [](const char *text) { DistPlan R; R.error = text; return R; };
  if (!map.p || !dist.p) return refuse("null argument");
  if (target != DT_TO_NONZERO && target != DT_TO_ZERO) return refuse("target must be HC_DT_TO_NONZERO or HC_DT_TO_ZERO");
  if (dist_type != DT_SQUARED_I32 && dist_type != DT_F32) return refuse("dist_type must be HC_DT_SQUARED_I32 or HC_DT_F32");
  if (n < 1 || n > max_frames) return refuse("nframes out of range");
  if (n > 65535) return refuse("more than 65535 frames in one call");
  if (W < 1 || H < 1) return refuse("width and height must be positive");
  if ((long long)W * H >= 0x7FFFFFFFll) return refuse("width * height reaches 2^31 - 1 pixels");
  if ((long long)(W - 1) * (W - 1) + (long long)(H - 1) * (H - 1) >= 0x7FFFFFFFll) return refuse("the squared diagonal (W - 1)^2 + (H - 1)^2 reaches 2^31 - 1");
  if (W > DT_MAX_W) return refuse("width above the 16384 columns of the row k_dt_rows keeps in LDS");
  if (const ViewFault f = check_view(map, (size_t)W, H, n, 1, true)) return refuse(VIEW_FAULT_TEXT[f]);
  if (const ViewFault f = check_view(dist, 4 * (size_t)W, H, n, 4, true))
    return refuse(f == VIEW_ALIGN ? "d_dist, dist_pitch and dist_frame_stride must be multiples of 4" : f == VIEW_PITCH ? "dist_pitch smaller than a row of 4-byte distances" : VIEW_FAULT_TEXT[f]);
  if (nearest.p)
    if (const ViewFault f = check_view(nearest, 4 * (size_t)W, H, n, 4, true))
      return refuse(f == VIEW_ALIGN ? "d_nearest, nearest_pitch and nearest_frame_stride must be multiples of 4" : f == VIEW_PITCH ? "nearest_pitch smaller than a row of int32 indices" : VIEW_FAULT_TEXT[f]);
  uintptr_t end[3] = { 0, 0, 0 };
  if (!view_end(map, (size_t)W, H, n, &end[0]) || !view_end(dist, 4 * (size_t)W, H, n, &end[1]) || (nearest.p && !view_end(nearest, 4 * (size_t)W, H, n, &end[2])))
    return refuse("a view wraps the address space");
  if (map.p < end[1] && dist.p < end[0]) return refuse("the map and the distance plane overlap");
  if (nearest.p && map.p < end[2] && nearest.p < end[0]) return refuse("the map and the nearest plane overlap");
  // The two outputs may be ROIs of one plane side by side: the same pitch and frame stride, bases in one row of that plane, rows
  // that do not meet.  Their byte ranges interleave then, but they share no byte (rows r and r' of frames f and f' lie in different
  // rows of the plane unless r = r' and f = f': a frame stride holds a frame).
  const size_t word_row = 4 * (size_t)W, apart = (size_t)(dist.p < nearest.p ? nearest.p - dist.p : dist.p - nearest.p);
  const bool side_by_side = nearest.p && dist.pitch == nearest.pitch && (n == 1 || dist.fs == nearest.fs) && apart >= word_row && apart <= dist.pitch - word_row;
  if (nearest.p && !side_by_side && dist.p < end[2] && nearest.p < end[1]) return refuse("the distance plane and the nearest plane overlap");
  DistParams &d = P.dp;
  d.map = (const uint8_t *)map.p; d.pitch = map.pitch; d.frame_stride = map.fs;
  d.dist = (int32_t *)dist.p; d.dist_pitch = dist.pitch; d.dist_frame_stride = dist.fs;
  if (nearest.p) { d.nearest = (int32_t *)nearest.p; d.nearest_pitch = nearest.pitch; d.nearest_frame_stride = nearest.fs; }
  d.W = W; d.H = H; d.nframes = n; d.target = target; d.dist_type = dist_type;
  d.col_groups = (unsigned)((W + DT_COL_THREADS * DT_COLS_PER_LANE - 1) / (DT_COL_THREADS * DT_COLS_PER_LANE));
  d.row_groups = (unsigned)((H + DT_ROWS - 1) / DT_ROWS);
  d.lds_bytes = 4u * (unsigned)W;
  return P;
}

// ---- hc_thinning_device ---------------------------------------------------------------------------
static_assert(THIN_ZHANGSUEN == HC_THIN_ZHANGSUEN && THIN_GUOHALL == HC_THIN_GUOHALL, "canny_params.h names the header's methods");
// Everything the entry refuses and decides, but for the context pointer.  A call is, per pass, the zeroing of the removal tables,
// k_thin_pack, 2 * max_iterations launches of k_thin_step and k_thin_unpack.  The context's scratch holds, per frame of a pass,
// two bit planes of H rows of row_words dwords and a table of max_iterations + 1 removal words (frame_bytes in all), laid out
// [plane A x frames_per_pass][plane B x frames_per_pass][tables x frames_per_pass].  It falls under the context's scratch bound: a
// batch is cut into passes of as many whole frames as fit.  pack / step / unpack describe the first pass with null scratch
// pointers; thin_pass gives the blocks of pass k.  A refused plan holds nothing but its text.
struct ThinPlan {
  const char *error = nullptr;
  ThinPackParams pack{};
  ThinStepParams step{};
  ThinUnpackParams unpack{};
  int method = 0, max_iterations = 0;
  int row_words = 0, tile_rows = 0, tiles = 0, panels = 0;
  int frames = 0, frames_per_pass = 0, passes = 0;
  size_t plane_bytes = 0, table_bytes = 0, frame_bytes = 0, scratch_bytes = 0;
};
inline ThinPlan plan_thinning(int W, int H, bool per_channel, int max_batch, const View &in, const View &out, int n, int method, int max_iterations, uintptr_t status,
                              size_t scratch_bound)
{
  ThinPlan P;
  auto refuse = [](const char *text) { ThinPlan R; R.error = text; return R; };
  if (!in.p || !out.p) return refuse("null argument");
  if (method != THIN_ZHANGSUEN && method != THIN_GUOHALL) return refuse("method must be HC_THIN_ZHANGSUEN or HC_THIN_GUOHALL");
  if (max_iterations < 1 || max_iterations > THIN_MAX_ITERATIONS) return refuse("max_iterations outside 1..1024");
  if (status & 3u) return refuse("d_status must be 4-byte aligned");
  if (W < 1 || H < 1) return refuse("width and height must be positive");
  if (n < 1 || n > max_batch * (per_channel ? 3 : 1)) return refuse("nframes out of range");
  const size_t row = (size_t)W;
  for (const View *v : { &in, &out })
    if (const ViewFault f = check_view(*v, row, H, n, 1, true)) return refuse(VIEW_FAULT_TEXT[f]);
  uintptr_t end[2];
  if (!view_end(in, row, H, n, &end[0]) || !view_end(out, row, H, n, &end[1])) return refuse("a view wraps the address space");
  if (in.p < end[1] && out.p < end[0]) return refuse("the map and the output view overlap (in-place operation is not supported)");
  P.method = method; P.max_iterations = max_iterations;
  P.row_words = thin_row_words(W); P.tile_rows = THIN_TILE_ROWS; P.tiles = thin_tiles(H); P.panels = thin_panels(W);
  // (H * pitch < 2^32 and pitch >= W: a plane is below 2^29 + 4 H bytes, so the sums below do not wrap)
  P.plane_bytes = (size_t)H * P.row_words * 4;
  P.table_bytes = 4 * ((size_t)max_iterations + 1);
  P.frame_bytes = 2 * P.plane_bytes + P.table_bytes;
  if (scratch_bound < P.frame_bytes) return refuse("one frame of bit planes exceeds the context's scratch bound");
  P.frames = n;
  P.frames_per_pass = (int)std::min<size_t>((size_t)n, scratch_bound / P.frame_bytes);
  P.passes = (n + P.frames_per_pass - 1) / P.frames_per_pass;
  P.scratch_bytes = (size_t)P.frames_per_pass * P.frame_bytes;
  if ((long long)P.frames_per_pass * P.panels * P.tiles > 0x7FFFFFF0ll || P.plane_bytes > 0xFFFFFFFCull) return refuse("too many work items (frames of a pass x panels x row tiles)");
  ThinPackParams &a = P.pack;
  a.map = (const uint8_t *)in.p; a.pitch = in.pitch; a.frame_stride = in.fs;
  a.plane_words = P.plane_bytes / 4;
  a.W = W; a.H = H; a.nframes = P.frames_per_pass; a.row_words = P.row_words; a.segs = thin_segs(W);
  a.in_aligned = aligned4(in.p, in.pitch, in.fs);
  ThinStepParams &s = P.step;
  s.plane_words = a.plane_words;
  s.H = H; s.nframes = P.frames_per_pass; s.row_words = P.row_words; s.npanels = P.panels; s.ntiles = P.tiles;
  s.total_items = s.nframes * s.npanels * s.ntiles;
  s.table_words = max_iterations + 1; s.method = method;
  ThinUnpackParams &u = P.unpack;
  u.status = (u32 *)status;
  u.out = (uint8_t *)out.p; u.out_pitch = out.pitch; u.out_frame_stride = out.fs;
  u.plane_words = a.plane_words;
  u.W = W; u.H = H; u.nframes = P.frames_per_pass; u.row_words = P.row_words; u.segs = a.segs;
  u.out_aligned = aligned4(out.p, out.pitch, out.fs);
  u.table_words = s.table_words; u.max_iterations = max_iterations;
  return P;
}

// The launches of pass k of a plan that was not refused (0 <= k < passes): the blocks of k_thin_pack, k_thin_step (every
// sub-iteration and iteration takes the same) and k_thin_unpack, and the tables the pass zeroes first; scratch: scratch_bytes,
// 4-byte aligned
struct ThinPass { ThinPackParams pack; ThinStepParams step; ThinUnpackParams unpack; uintptr_t tables; size_t tables_bytes; };
inline ThinPass thin_pass(const ThinPlan &P, int k, uintptr_t scratch)
{
  ThinPass R{ P.pack, P.step, P.unpack, 0, 0 };
  const int f0 = k * P.frames_per_pass, nf = std::min(P.frames_per_pass, P.frames - f0);
  const size_t planes = (size_t)P.frames_per_pass * P.plane_bytes;
  u32 *const A = (u32 *)scratch, *const B = (u32 *)(scratch + planes), *const T = (u32 *)(scratch + 2 * planes);
  R.tables = (uintptr_t)T; R.tables_bytes = (size_t)nf * P.table_bytes;
  R.pack.map += (size_t)f0 * R.pack.frame_stride;
  R.pack.plane_a = A; R.pack.nframes = nf;
  R.step.plane_a = A; R.step.plane_b = B; R.step.removed = T; R.step.nframes = nf;
  R.step.total_items = nf * R.step.npanels * R.step.ntiles;
  R.unpack.plane_a = A; R.unpack.removed = T; R.unpack.nframes = nf;
  R.unpack.out += (size_t)f0 * R.unpack.out_frame_stride;
  if (R.unpack.status) R.unpack.status += 2 * (size_t)f0;
  return R;
}

// ---- hc_corner_response_device --------------------------------------------------------------------
static_assert(CORNER_MIN_EIGEN == HC_CORNER_MIN_EIGEN && CORNER_HARRIS == HC_CORNER_HARRIS, "canny_params.h names the header's methods");
// Everything the entry refuses and decides, but for the context pointer: one launch of k_corner_response, no scratch, no passes.
// A refused plan holds nothing but its text.
struct CornerPlan { const char *error = nullptr; CornerParams cp{}; };
inline CornerPlan plan_corner_response(int W, int H, int max_frames, const View &dx, uintptr_t dy, const View &out, int n, int block_size, int method, double harris_k)
{
  CornerPlan P;
  auto refuse = [](const char *text) { CornerPlan R; R.error = text; return R; };
  if (!dx.p || !dy || !out.p) return refuse("null argument");
  if (!corner_block_ok(block_size)) return refuse("block_size must be 3, 5 or 7");
  if (method != CORNER_MIN_EIGEN && method != CORNER_HARRIS) return refuse("method must be HC_CORNER_MIN_EIGEN or HC_CORNER_HARRIS");
  if (method == CORNER_HARRIS && !std::isfinite(harris_k)) return refuse("harris_k must be finite");
  if (W < 1 || H < 1) return refuse("width and height must be positive");
  if (n < 1 || n > max_frames) return refuse("nframes out of range");
  const size_t row16 = 2 * (size_t)W, row32 = 4 * (size_t)W;
  const View dyv{ dy, dx.pitch, dx.fs };
  if (const ViewFault f = check_view(dx, row16, H, n, 2, true)) return refuse(VIEW_FAULT_TEXT[f]);
  if (const ViewFault f = check_view(dyv, row16, H, n, 2, true)) return refuse(VIEW_FAULT_TEXT[f]);
  if (const ViewFault f = check_view(out, row32, H, n, 4, true)) return refuse(f == VIEW_ALIGN ? "d_response, out_pitch and out_frame_stride must be multiples of 4" : VIEW_FAULT_TEXT[f]);
  uintptr_t ex = 0, ey = 0, eo = 0;
  if (!view_end(dx, row16, H, n, &ex) || !view_end(dyv, row16, H, n, &ey) || !view_end(out, row32, H, n, &eo)) return refuse("a view wraps the address space");
  if ((dx.p < eo && out.p < ex) || (dy < eo && out.p < ey)) return refuse("a derivative plane and the response view overlap");
  CornerParams &c = P.cp;
  c.dx = (const uint8_t *)dx.p; c.dy = (const uint8_t *)dy; c.pitch = dx.pitch; c.frame_stride = dx.fs;
  c.out = (uint8_t *)out.p; c.out_pitch = out.pitch; c.out_frame_stride = out.fs;
  c.W = W; c.H = H; c.nframes = n; c.block_size = block_size; c.method = method;
  c.k = method == CORNER_HARRIS ? (float)harris_k : 0.0f;
  const uintptr_t ia = dx.p | dy | dx.pitch | dx.fs, oa = out.p | out.pitch | out.fs;
  c.in_align = (ia & 7u) == 0 ? 8 : (ia & 3u) == 0 ? 4 : 2;
  c.out_align = (oa & 15u) == 0 ? 16 : (oa & 7u) == 0 ? 8 : 4;
  c.nstrips = corner_strips(W); c.nchunks = corner_chunks(H);
  const long long items = (long long)n * c.nstrips * c.nchunks;
  if (items > 0x7FFFFFF0ll) return refuse("too many work items (nframes x strips x row chunks)");
  c.total_items = (int)items;
  return P;
}

// ---- hc_good_features_device ----------------------------------------------------------------------
// The smallest int64 whose double is >= min_distance^2, capped at 2^62 as hough_circle_geometry caps its own (no two pixels lie
// 2^62 apart: a larger bound is that one).  min_distance finite and >= 0.
inline long long feat_min_d2(double min_distance)
{
  const double v = min_distance * min_distance;
  return v >= 4611686018427387904.0 ? (1ll << 62) : (long long)std::ceil(v);
}
// Everything the entry refuses and decides, but for the context pointer.  A call is, per pass, the zeroing of the histograms and
// state words and one launch_good_features.  The context's scratch holds, per frame of a pass, the ranked and kept lists (16 bytes
// a candidate each), the candidate list (8 bytes), the histogram, the state words and two words a row: O(candidate_capacity + rows
// + bins), no plane.  It falls under the context's scratch bound: a batch is cut into passes of as many whole frames as fit.  fp
// describes the first pass with null scratch pointers; feat_pass gives pass k.  A refused plan holds nothing but its text.
struct FeatPlan {
  const char *error = nullptr;
  FeatParams fp{};
  int frames = 0, frames_per_pass = 0, passes = 0;
  size_t frame_list_bytes = 0, frame_cand_bytes = 0, frame_hist_bytes = 0, frame_state_bytes = 0, frame_rows_bytes = 0, frame_bytes = 0, scratch_bytes = 0;
};
inline FeatPlan plan_good_features(int W, int H, int max_frames, const View &plane, int n, double quality_level, double min_distance, size_t candidate_capacity,
                                   uintptr_t counts, uintptr_t corners, uintptr_t quality, size_t corner_capacity, size_t scratch_bound)
{
  FeatPlan P;
  auto refuse = [](const char *text) { FeatPlan R; R.error = text; return R; };
  if (!plane.p || !counts) return refuse("null argument");
  if (corner_capacity && !corners) return refuse("d_corners is null with corner_capacity > 0");
  if (counts & 3u) return refuse("d_corner_counts must be 4-byte aligned");
  if (corners & 7u) return refuse("d_corners must be 8-byte aligned");
  if (quality & 3u) return refuse("d_quality must be 4-byte aligned");
  if (!std::isfinite(quality_level) || !(quality_level > 0) || quality_level > 1) return refuse("quality_level must lie in (0, 1]");
  if (!std::isfinite(min_distance) || min_distance < 0) return refuse("min_distance must be finite and not negative");
  if (candidate_capacity < 1 || candidate_capacity > (size_t)FEAT_MAX_CANDIDATES) return refuse("candidate_capacity must lie in 1 .. 4096");
  if (W < 1 || H < 1) return refuse("width and height must be positive");
  if (n < 1 || n > max_frames) return refuse("nframes out of range");
  if (const ViewFault f = check_view(plane, 4 * (size_t)W, H, n, 4, true)) return refuse(f == VIEW_ALIGN ? "d_response, pitch and frame_stride must be multiples of 4" : VIEW_FAULT_TEXT[f]);
  uintptr_t end = 0;
  if (!view_end(plane, 4 * (size_t)W, H, n, &end)) return refuse("a view wraps the address space");
  if (corner_capacity > SIZE_MAX / 8 / (size_t)n) return refuse("corner_capacity * 8 * nframes overflows size_t");
  P.frame_list_bytes = candidate_capacity * 16; P.frame_cand_bytes = candidate_capacity * 8;
  P.frame_hist_bytes = (size_t)FEAT_BINS * 4; P.frame_state_bytes = (size_t)FEAT_STATE_WORDS * 4; P.frame_rows_bytes = (size_t)H * 8;
  P.frame_bytes = 2 * P.frame_list_bytes + P.frame_cand_bytes + P.frame_hist_bytes + P.frame_state_bytes + P.frame_rows_bytes;
  if (scratch_bound < P.frame_bytes) return refuse("one frame's lists and tables exceed the context's scratch bound");
  P.frames = n;
  P.frames_per_pass = (int)std::min<size_t>(std::min<size_t>((size_t)n, scratch_bound / P.frame_bytes), HOUGH_MAX_PASS_FRAMES);
  P.passes = (n + P.frames_per_pass - 1) / P.frames_per_pass;
  P.scratch_bytes = (size_t)P.frames_per_pass * P.frame_bytes;
  FeatParams &f = P.fp;
  f.plane = (const uint8_t *)plane.p; f.pitch = plane.pitch; f.frame_stride = plane.fs;
  f.W = W; f.H = H; f.nframes = P.frames_per_pass; f.ngroups = feat_groups(H);
  f.quality = (float)quality_level; f.min_d2 = feat_min_d2(min_distance);
  f.candidate_capacity = (int)candidate_capacity; f.corner_capacity = corner_capacity;
  f.counts = (u32 *)counts; f.corners = (float *)corners; f.quality_out = (float *)quality;
  return P;
}

// Pass k of a plan that was not refused (0 <= k < passes), on `scratch` (scratch_bytes, 16-byte aligned): the sections lie in the
// order ranked | kept | candidates | histograms | state words | rows, the widest alignment first; [zero, zero + zero_bytes) is
// what the pass zeroes first: the histograms and the state words of its frames (the two sections are neighbours)
struct FeatPass { FeatParams fp; uintptr_t zero; size_t zero_bytes; };
inline FeatPass feat_pass(const FeatPlan &P, int k, uintptr_t scratch)
{
  FeatPass R{ P.fp, 0, 0 };
  FeatParams &f = R.fp;
  const int f0 = k * P.frames_per_pass;
  const size_t fpp = (size_t)P.frames_per_pass;
  f.nframes = std::min(P.frames_per_pass, P.frames - f0);
  f.plane += (size_t)f0 * f.frame_stride;
  f.counts += f0;
  if (f.corners) f.corners += (size_t)f0 * f.corner_capacity * 2;
  if (f.quality_out) f.quality_out += (size_t)f0 * f.corner_capacity;
  uintptr_t q = scratch;
  f.ranked = (int32_t *)q; q += fpp * P.frame_list_bytes;
  f.kept = (int32_t *)q;   q += fpp * P.frame_list_bytes;
  f.cand = (u32 *)q;       q += fpp * P.frame_cand_bytes;
  f.hist = (u32 *)q;       q += fpp * P.frame_hist_bytes;
  f.state = (u32 *)q;      q += fpp * P.frame_state_bytes;
  f.rows = (u32 *)q;
  R.zero = (uintptr_t)f.hist;
  R.zero_bytes = fpp * P.frame_hist_bytes + (size_t)f.nframes * P.frame_state_bytes;
  return R;
}

// ---- hc_pyr_down_device ---------------------------------------------------------------------------
// Everything the entry refuses and decides, but for the context pointer: one launch of k_pyr_down8, no scratch, no passes.  The
// planes are sw x sh, a level of the context's W x H frame: 3 <= sw <= W, 3 <= sh <= H.  A refused plan holds nothing but its text.
struct PyrPlan { const char *error = nullptr; PyrParams pp{}; };
inline PyrPlan plan_pyr_down(int W, int H, int max_frames, const View &src, int sw, int sh, const View &dst, int n)
{
  PyrPlan P;
  auto refuse = [](const char *text) { PyrPlan R; R.error = text; return R; };
  if (!src.p || !dst.p) return refuse("null argument");
  if (sw < PYR_MIN_SIDE || sh < PYR_MIN_SIDE) return refuse("src_width and src_height must be 3 at least");
  if (sw > W || sh > H) return refuse("src_width and src_height must not exceed the context's frame");
  if (n < 1 || n > max_frames) return refuse("nframes out of range");
  const int dw = pyr_half(sw), dh = pyr_half(sh);
  if (const ViewFault f = check_view(src, (size_t)sw, sh, n, 1, true)) return refuse(VIEW_FAULT_TEXT[f]);
  if (const ViewFault f = check_view(dst, (size_t)dw, dh, n, 1, true)) return refuse(f == VIEW_PITCH ? "dst_pitch smaller than a destination row" : f == VIEW_STRIDE ? "dst_frame_stride below the destination height * dst_pitch" : VIEW_FAULT_TEXT[f]);
  uintptr_t es = 0, ed = 0;
  if (!view_end(src, (size_t)sw, sh, n, &es) || !view_end(dst, (size_t)dw, dh, n, &ed)) return refuse("a view wraps the address space");
  if (src.p < ed && dst.p < es) return refuse("the source and destination views overlap");
  PyrParams &q = P.pp;
  q.in = (const uint8_t *)src.p; q.in_pitch = src.pitch; q.in_frame_stride = src.fs;
  q.out = (uint8_t *)dst.p; q.out_pitch = dst.pitch; q.out_frame_stride = dst.fs;
  q.W = sw; q.H = sh; q.dW = dw; q.dH = dh; q.nframes = n;
  q.in_aligned = aligned4(src.p, src.pitch, src.fs); q.out_aligned = ((dst.p | dst.pitch | dst.fs) & 1u) == 0;
  q.nstrips = pyr_strips(sw); q.nchunks = pyr_chunks(dh);
  const long long items = (long long)n * q.nstrips * q.nchunks;
  if (items > 0x7FFFFFF0ll) return refuse("too many work items (nframes x strips x row chunks)");
  q.total_items = (int)items;
  return P;
}

// ---- hc_lk_flow_device ----------------------------------------------------------------------------
// Everything the entry refuses and decides, but for the context pointer: one launch of k_lk_flow, a wave per point slot, no scratch.
// The planes are w x h, a level of the context's frame: 1 <= w <= W, 1 <= h <= H.  A refused plan holds nothing but its text.
struct FlowPlan { const char *error = nullptr; FlowParams fp{}; };
inline FlowPlan plan_lk_flow(int W, int H, int max_frames, const View &prev, uintptr_t next, int w, int h, int level, int n, uintptr_t counts, uintptr_t prev_pts,
                             uintptr_t next_pts, size_t capacity, int win, int max_iterations, double epsilon, double min_eig_threshold, int use_initial,
                             uintptr_t status, uintptr_t err)
{
  FlowPlan P;
  auto refuse = [](const char *text) { FlowPlan R; R.error = text; return R; };
  if (!prev.p || !next || !counts || !prev_pts || !next_pts || !status) return refuse("null argument");
  if ((counts | prev_pts | next_pts | err) & 3u) return refuse("d_counts, d_prev_pts, d_next_pts and d_err must be 4-byte aligned");
  if (level < 0 || level > FLOW_MAX_LEVEL) return refuse("level must lie in 0 .. 15");
  if (!flow_win_ok(win)) return refuse("win must be odd and lie in 5 .. 31");
  if (max_iterations < 1 || max_iterations > FLOW_MAX_ITERATIONS) return refuse("max_iterations must lie in 1 .. 64");
  if (!std::isfinite(epsilon) || epsilon < 0) return refuse("epsilon must be finite and not negative");
  if (!std::isfinite(min_eig_threshold) || min_eig_threshold < 0) return refuse("min_eig_threshold must be finite and not negative");
  if (w < 1 || h < 1) return refuse("width and height must be positive");
  if (w > W || h > H) return refuse("width and height must not exceed the context's frame");
  if (n < 1 || n > max_frames) return refuse("nframes out of range");
  if (capacity < 1) return refuse("capacity must be positive");
  if (capacity > SIZE_MAX / 8 / (size_t)n) return refuse("capacity * 8 * nframes overflows size_t");
  if (capacity > ((size_t)1 << 30)) return refuse("capacity above 2^30 (a wave per point slot)");
  const View nextv{ next, prev.pitch, prev.fs };
  if (const ViewFault f = check_view(prev, (size_t)w, h, n, 1, true)) return refuse(VIEW_FAULT_TEXT[f]);
  if (const ViewFault f = check_view(nextv, (size_t)w, h, n, 1, true)) return refuse(VIEW_FAULT_TEXT[f]);
  uintptr_t ep = 0, en = 0;
  if (!view_end(prev, (size_t)w, h, n, &ep) || !view_end(nextv, (size_t)w, h, n, &en)) return refuse("a view wraps the address space");
  const size_t pts_bytes = capacity * 8 * (size_t)n;
  if (next_pts > UINTPTR_MAX - pts_bytes || prev_pts > UINTPTR_MAX - pts_bytes || counts > UINTPTR_MAX - 4 * (size_t)n) return refuse("a view wraps the address space");
  const uintptr_t o0 = next_pts, o1 = next_pts + pts_bytes;
  if (prev_pts < o1 && o0 < prev_pts + pts_bytes) return refuse("d_next_pts overlaps d_prev_pts");
  if (counts < o1 && o0 < counts + 4 * (size_t)n) return refuse("d_next_pts overlaps d_counts");
  if ((prev.p < o1 && o0 < ep) || (next < o1 && o0 < en)) return refuse("d_next_pts overlaps an image");
  FlowParams &f = P.fp;
  f.prev = (const uint8_t *)prev.p; f.next = (const uint8_t *)next; f.pitch = prev.pitch; f.frame_stride = prev.fs;
  f.W = w; f.H = h; f.level = level; f.nframes = n;
  f.counts = (const u32 *)counts; f.prev_pts = (const float *)prev_pts; f.next_pts = (float *)next_pts; f.capacity = capacity;
  f.win = win; f.max_iterations = max_iterations; f.use_initial = use_initial ? 1 : 0;
  f.eps2 = (float)(epsilon * epsilon); f.min_eig = (float)min_eig_threshold;
  f.status = (uint8_t *)status; f.err = (float *)err;
  f.groups = (u32)((capacity + FLOW_WAVES - 1) / FLOW_WAVES);
  return P;
}

}  // namespace hc
