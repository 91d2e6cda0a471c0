// hipcanny.hip -- host side of libhipcanny.so: the C ABI declared in include/hipcanny.h.
// Replaces the host half of the reference operator (src/cvp/cannyEdgeH.cu): allocation, upload,
// the stage switch of CannyEdge::run, the hysteresis launch loop and the output copy.
// This file owns the context and queues the GPU work; what a run does is decided in host_plan.h (plan_front, plan_hyst).
// There is no CPU fallback anywhere in this file: without a gfx950 device hc_create fails.
#include "hc_context.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

using namespace hc;

thread_local std::string hc::g_err;  // (declared in hc_context.h: device_ops.hip and legacy_front.hip fail through it too)

namespace {
// the two copy streams all HC_OPT_COPY_STREAMS contexts of a device share (created on first use, kept for the process)
constexpr int MAX_DEVICES = 64;
hipStream_t g_h2d[MAX_DEVICES] = { nullptr }, g_d2h[MAX_DEVICES] = { nullptr };
std::mutex g_copy_streams_mutex;  // contexts of different host threads may ask for them at the same time

// Internal frame buffers.  Rows of whole 16-byte groups are stored TIGHT (pitch = row bytes): a batch is then one contiguous
// block, and hc_upload / hc_download move it with a single 1-D DMA instead of a strided 2-D copy per frame (16 frames of
// 1080p over PCIe: 23.8 -> ~50 GB/s each way, bench.py host_fed).  Other widths keep rows padded to 256 bytes, which
// also gives the 8-px kernels the whole pixel groups they load.
int alloc_frames(uint8_t **ptr, size_t *pitch, size_t *fs, size_t row_bytes, int H, int n, size_t tight_row_bytes = 0)
{
  *pitch = frame_pitch(row_bytes, tight_row_bytes);
  *fs = *pitch * (size_t)H;
  HIPCK(hipMalloc((void **)ptr, *fs * (size_t)n));
  return HC_OK;
}

int ensure_stage_scratch(hc_ctx *c)
{
  if (c->d_blur) return HC_OK;
  const size_t n = (size_t)c->max_batch;
  HIPCK(hipMalloc((void **)&c->d_blur, c->out_fs * n));
  HIPCK(hipMalloc((void **)&c->d_nms, c->out_fs * n));
  HIPCK(hipMalloc((void **)&c->d_sx, c->out_fs * n * 2));
  HIPCK(hipMalloc((void **)&c->d_sy, c->out_fs * n * 2));
  return HC_OK;
}

int alloc_slot_parts(hc_ctx *c, Slot &s)
{
  const size_t out_frames = (size_t)c->max_batch * (c->per_channel ? 3 : 1);
  const size_t plane_bytes = sizeof(u32) * (size_t)c->RD * c->H * out_frames;
  HIPCK(hipMalloc((void **)&s.d_sbits, plane_bytes));
  HIPCK(hipMalloc((void **)&s.d_cbits, plane_bytes));
  // row padding beyond the strips' bytes is never written by the kernels and must read as 0.
  // Cleared ON THE CONTEXT STREAM and waited for: slots 1..3 are allocated inside a run, with other runs in flight, and the
  // front kernel that fills these planes is queued on c->stream a few microseconds later.  A plain hipMemset goes to the
  // null stream, which the context's non-blocking streams do not wait for, and a device memset need not be complete when
  // the call returns: a clear that lands after the front kernel wipes the candidate bits of the slot's first run.
  HIPCK(hipMemsetAsync(s.d_sbits, 0, plane_bytes, c->stream));
  HIPCK(hipMemsetAsync(s.d_cbits, 0, plane_bytes, c->stream));
  HIPCK(hipStreamSynchronize(c->stream));
  s.wl_cap = slot_wl_cap(out_frames, c->H, c->RD);
  HIPCK(hipMalloc((void **)&s.d_wl_list, sizeof(u32) * 2 * s.wl_cap));
  HIPCK(hipMalloc((void **)&s.d_flags, sizeof(u32) * run_flag_words(s.wl_cap)));
  HIPCK(hipHostMalloc((void **)&s.h_flags, sizeof(u32) * (FLAG_WORDS + WL_COUNT_WORDS), hipHostMallocDefault));
  {
    // the hysteresis launches are few, small and dependent (latency-bound); at the highest priority their workgroups are
    // placed ahead of the next run's 30k-wave front kernel instead of behind it
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    HIPCK(hipStreamCreateWithPriority(&s.s_hyst, hipStreamNonBlocking, greatest));
  }
  HIPCK(hipEventCreateWithFlags(&s.ev_front, hipEventDisableTiming));  // (cross-stream waits only: the timestamps watch_chain compares are ring.f / ring.d)
  HIPCK(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
  return HC_OK;
}

void free_slot(Slot &s)
{
  for (void *q : { (void *)s.d_sbits, (void *)s.d_cbits, (void *)s.d_wl_list, (void *)s.d_flags }) (void)hipFree(q);
  if (s.h_flags) (void)hipHostFree(s.h_flags);
  if (s.ev_front) (void)hipEventDestroy(s.ev_front);
  if (s.ev_done) (void)hipEventDestroy(s.ev_done);
  if (s.s_hyst) (void)hipStreamDestroy(s.s_hyst);
  s = Slot{};
}

// A slot is either complete or empty: slots 1..3 are allocated lazily inside a run, and a run that found d_sbits set
// but the stream or the flag words missing would memset a null pointer and queue its hysteresis on the null stream.
int alloc_slot(hc_ctx *c, Slot &s)
{
  if (s.complete) return HC_OK;
  const int rc = alloc_slot_parts(c, s);
  if (rc != HC_OK) {
    const std::string why = g_err;
    free_slot(s);
    return fail(rc, why);
  }
  s.complete = true;
  return HC_OK;
}

#ifdef HC_LEGACY_FRONT
// split mode: blur plane [frames][strip][H][256 B] (see canny_kernels.hip); every byte k_nms reads is written by k_blur
int ensure_blur_plane(hc_ctx *c)
{
  const size_t frames = (size_t)c->max_batch * (c->per_channel ? 3 : 1);
  if (c->d_bplane && c->bplane_frames == frames) return HC_OK;
  if (c->d_bplane) { (void)hipFree(c->d_bplane); c->d_bplane = nullptr; }
  c->bplane_fs = (size_t)c->nstrips * c->H * 256;
  HIPCK(hipMalloc((void **)&c->d_bplane, c->bplane_fs * frames));
  c->bplane_frames = frames;
  return HC_OK;
}
#endif

// k_front8's dump areas and page of zeros.  big: sized for the HALF form, whose half-wave B reaches its frame through lane
// offsets of up to one frame stride (three bit-plane / output frames in per-channel mode)
int alloc_dump(hc_ctx *c, bool big)
{
  if (c->d_dump && (c->dump_region != 0) == big) return HC_OK;
  if (c->d_dump) { (void)hipFree(c->d_dump); c->d_dump = nullptr; }
  size_t bytes = 16384 + 32768;
  c->dump_region = 0;
  if (big) {
    c->dump_region = half_dump_region(c->in_fs, c->out_fs, c->RD, c->H);
    bytes = 4 * c->dump_region;
  }
  HIPCK(hipMalloc((void **)&c->d_dump, bytes));
  HIPCK(hipMemset(c->d_dump, 0, bytes));
  return HC_OK;
}

int ensure_debug_buffers(hc_ctx *c)
{
  if (c->dbg.s) return HC_OK;
  const size_t frames = (size_t)c->max_batch * (c->per_channel ? 3 : 1);
  const size_t plane_bytes = sizeof(u32) * (size_t)c->RD * c->H * frames;
  HIPCK(hipMalloc((void **)&c->dbg.s, plane_bytes));
  HIPCK(hipMalloc((void **)&c->dbg.c, plane_bytes));
  HIPCK(hipMalloc((void **)&c->dbg.blur, c->out_fs * frames));
  return HC_OK;
}

void free_debug_buffers(hc_ctx *c)
{
  for (void *q : { (void *)c->dbg.s, (void *)c->dbg.c, (void *)c->dbg.blur }) (void)hipFree(q);
  c->dbg.s = c->dbg.c = nullptr;
  c->dbg.blur = nullptr;
  c->dbg.frames = 0;
}

int copy_frames_d2d(hc_ctx *c, hipStream_t st, void *dst, size_t dpitch, size_t dfs, const void *src, size_t spitch, size_t sfs, size_t row_bytes, int n)
{
  // a kernel, not hipMemcpy2DAsync: its row-by-row DMA took 1.5 - 2.5 ms for 512 frames of 1918 x 1079 (k_copy_rows: 0.3 ms)
  for (int f0 = 0; f0 < n; f0 += 65535) {
    const int nf = std::min(n - f0, 65535);
    HIPCK(launch_copy_rows((uint8_t *)dst + dfs * f0, dpitch, dfs, (const uint8_t *)src + sfs * f0, spitch, sfs, row_bytes, c->H, nf, st));
  }
  return HC_OK;
}

// n maps of the internal output buffer to the caller's view (out_view_staged), on st.  remember: a host-side continuation of
// the run in slot s rewrites the maps and repeats the copy (finish_slot)
int copy_out_staged(hc_ctx *c, Slot &s, hipStream_t st, void *out, size_t out_pitch, size_t out_fs, int n, bool remember)
{
  if (int rc = copy_frames_d2d(c, st, out, out_pitch, out_fs, c->d_out, c->out_pitch, c->out_fs, (size_t)c->W, n)) return rc;
  if (remember) { s.copy_dst = out; s.copy_pitch = out_pitch; s.copy_fs = out_fs; }
  return HC_OK;
}

// Feeds ChainWatch (host_plan.h) when run i is complete: the chain of run i-1 ran beside the front kernel of run i, and
// the timestamps of all three events involved -- end of front i-1, end of chain i-1, end of front i -- can be read.
void watch_chain(hc_ctx *c, const Slot &s)
{
  if (!s.seq || s.stream == c->stream || c->nslot_use >= NSLOT) return;
  const unsigned long long i = s.seq;
  const int a = (int)((i - 1) & 7), b = (int)(i & 7);
  if (c->ring.seq[b] != i || c->ring.seq[a] != i - 1 || i < 2) return;
  float front_ms = 0.0f, lead_ms = 0.0f;  // front kernel i (end to end); end of chain i-1 -> end of front kernel i
  if (hipEventElapsedTime(&front_ms, c->ring.f[a], c->ring.f[b]) != hipSuccess || hipEventElapsedTime(&lead_ms, c->ring.d[a], c->ring.f[b]) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  c->watch.update(i, c->nslot_use, front_ms, lead_ms);
}

}  // namespace

// (namespace hc, declared in hc_context.h: device_ops.hip completes the writers of a map it is about to read through it)
// Completes a queued fused run: waits for it, and if its queued hysteresis launches did not reach
// the fixpoint (flag of the last one still set -- adversarial inputs only), keeps iterating, then
// redoes the expand.
int hc::finish_slot(hc_ctx *c, Slot &s)
{
  if (!s.pending) return HC_OK;
  s.pending = false;
  s.out0 = s.out1 = 0;  // (this function only returns when the run is complete)
  hipStream_t st = s.stream;
  HIPCK(hipEventSynchronize(s.ev_done));
  watch_chain(c, s);
  const HystPlan &p = s.plan;
  const int K = p.K;
  int work = 0;
  for (int k = 0; k < K; ++k) work += s.h_flags[k] != 0;
  work = std::min(K, work + 1);
  std::memcpy(c->last.stats, s.h_flags + MAX_HYST_LAUNCHES, sizeof(c->last.stats));
  c->last.continued = 0;
  c->last.totals[0] += 1;
  c->last.totals[3] += (unsigned long long)K;
  u32 wl_counts[MAX_HYST_LAUNCHES + 1];  // as the queued launches left them (a continuation reads h_flags again)
  std::memcpy(wl_counts, s.h_flags + FLAG_WORDS, sizeof(wl_counts));
  {  // diagnostics: the schedule this run got (read by hc_last_hysteresis_schedule; decides nothing)
    int *d = c->last.sched;
    d[HC_SCHED_LAUNCHES] = K; d[HC_SCHED_LISTS] = p.mixed ? 2 : p.lists0; d[HC_SCHED_LOOP] = p.loop ? 1 : 0;
    d[HC_SCHED_HIST_GRID] = d[HC_SCHED_LONGEST] = d[HC_SCHED_OVERFLOWS] = 0;
    for (int k = 1; k < K && !p.loop; ++k) {
      if (!p.served_list(k)) continue;
      const u32 len = wl_counts[k];
      d[HC_SCHED_LONGEST] = std::max(d[HC_SCHED_LONGEST], (int)std::min<u32>(len, 0x7FFFFFFFu));
      if (p.hist_grid(k) <= 0) continue;
      d[HC_SCHED_HIST_GRID] = d[HC_SCHED_HIST_GRID] ? std::min(d[HC_SCHED_HIST_GRID], p.hist_grid(k)) : p.hist_grid(k);
      if (len > (u32)p.hist_grid(k)) d[HC_SCHED_OVERFLOWS] += 1;
    }
    d[HC_SCHED_TILES] = (int)std::min<size_t>(p.wl_stride, 0x7FFFFFFF); d[HC_SCHED_TILE_ROWS] = p.tile_rows; d[HC_SCHED_WAVES] = p.waves;
    d[HC_SCHED_PANELS] = p.npanels; d[HC_SCHED_FRAMES] = s.ph.nframes;
  }
  const bool converged = s.h_flags[K - 1] == 0;
  if (!converged) {
    c->last.continued = 1;
    c->last.totals[1] += 1;
    if (c->dl.host) c->dl.stale = true;
    for (int round = 0; round < 1000000; ++round) {
      HIPCK(hipMemsetAsync(s.d_flags, 0, sizeof(u32) * run_flag_words(p.wl_stride), st));  // flags, worklist counts and reasons
      HystParams hp = s.ph;
      hp.late_grid = p.test_grid;  // (not the grids sized for the run's queued launches)
      hp.first_pass = 0;
      hp.stats = nullptr;
      for (int k = 0; k < K; ++k) {  // the schedule the run itself used
        hp.iter = k;
        hp.lists = p.lists[k];
        HIPCK(launch_hyst(hp, st));
      }
      HIPCK(hipMemcpyAsync(s.h_flags, s.d_flags, sizeof(u32) * (FLAG_WORDS + WL_COUNT_WORDS), hipMemcpyDeviceToHost, st));
      HIPCK(hipStreamSynchronize(st));
      for (int k = 0; k < K; ++k) work += s.h_flags[k] != 0;
      if (s.h_flags[K - 1] == 0) break;
    }
  }
  c->last.totals[2] += (unsigned long long)work;
  c->hist.finished(p, work, wl_counts);
  if (converged) return HC_OK;
  if (s.copy_dst)
    if (int rc = copy_frames_d2d(c, st, s.copy_dst, s.copy_pitch, s.copy_fs, s.ph.out, s.ph.out_pitch, s.ph.out_frame_stride, (size_t)c->W, s.n)) return rc;
  HIPCK(hipStreamSynchronize(st));
  return HC_OK;
}

namespace {

int finish_all(hc_ctx *c)
{
  // oldest first: slot `cur` is the next to be reused
  for (int k = 0; k < c->nslot_use; ++k)
    if (int rc = finish_slot(c, c->slot[(c->cur + k) % c->nslot_use])) return rc;
  for (Slot &q : c->slot)  // (slots of the other ring size hold nothing: the ring is drained before its size changes)
    if (int rc = finish_slot(c, q)) return rc;
  return HC_OK;
}

// bit planes of slot s -> fixpoint -> u8 image, queued on `st` by the schedule of plan_hyst
// zeroed_words: the front kernel of this run already zeroed that many words of s.d_flags (FrontParams::zero_words)
int queue_hyst_expand(hc_ctx *c, Slot &s, hipStream_t st, uint8_t *out, size_t out_pitch, size_t out_fs, int n, bool small_tiles, size_t zeroed_words = 0)
{
  s.plan = plan_hyst(c->RD, c->H, n, small_tiles, c->hopt, c->hist, s.wl_cap, zeroed_words);
  const HystPlan &p = s.plan;
  if (!p.fits) return fail(HC_E_ARG, "internal: hysteresis worklist capacity");
  HystParams hp{};
  hp.sbits = s.d_sbits; hp.cbits = s.d_cbits; hp.RD = c->RD; hp.H = c->H; hp.nframes = n; hp.flags = s.d_flags;
  hp.tile_rows = p.tile_rows; hp.waves = p.waves; hp.nrtiles = p.nrtiles; hp.npanels = p.npanels;
  hp.out = out; hp.out_pitch = out_pitch; hp.out_frame_stride = out_fs; hp.W = c->W;
  hp.wl_stride = p.wl_stride;
  hp.wl_count = s.d_flags + FLAG_WORDS;
  hp.wl_reason = s.d_flags + FLAG_WORDS + WL_COUNT_WORDS;
  hp.wl_list = s.d_wl_list;
  hp.first_pass = 1;
  hp.prov = s.prov ? 1 : 0;
  if (p.clear) HIPCK(hipMemsetAsync(s.d_flags, 0, sizeof(u32) * run_flag_words(p.wl_stride), st));
  if (p.loop) HIPCK(launch_hyst_loop(hp, p.K, s.d_flags + FLAG_WORDS + WL_COUNT_WORDS - 2, st));  // (the last two count words: unused by this form, zeroed with the flags)
  for (int k = p.loop ? p.K : 0; k < p.K; ++k) {
    hp.iter = k; hp.lists = p.lists[k]; hp.late_grid = p.late_grid[k];
    // diagnostics cost ~3 same-address atomics per wave (hundreds of microseconds per launch): opt-in only
    hp.stats = c->hopt.diag ? s.d_flags + MAX_HYST_LAUNCHES + 3 * k : nullptr;
    HIPCK(launch_hyst(hp, st));
  }
  HIPCK(hipMemcpyAsync(s.h_flags, s.d_flags, sizeof(u32) * (FLAG_WORDS + WL_COUNT_WORDS), hipMemcpyDeviceToHost, st));
  s.pending = true;
  s.ph = hp;
  s.n = n;
  s.stream = st;
  s.copy_dst = nullptr;
  return HC_OK;
}

// n maps of the internal output buffer to the host: tight rows on both sides are one contiguous block, one DMA; otherwise
// a 2-D copy per frame
int copy_out_d2h(hc_ctx *c, uint8_t *host, size_t row_stride, size_t frame_stride, int n, hipStream_t st)
{
  if (row_stride == (size_t)c->W && c->out_pitch == (size_t)c->W && frame_stride == c->out_fs)
    HIPCK(hipMemcpyAsync(host, c->d_out, c->out_fs * (size_t)n, hipMemcpyDeviceToHost, st));
  else
    for (int f = 0; f < n; ++f)
      HIPCK(hipMemcpy2DAsync(host + frame_stride * f, row_stride, c->d_out + c->out_fs * f, c->out_pitch, (size_t)c->W, (size_t)c->H, hipMemcpyDeviceToHost, st));
  return HC_OK;
}

// Pipelined runs: the slot of this run, after the run that used it nslot_use steps ago; a ring of another size is drained
// first.  Plain runs: slot 0, with nothing else in flight.
int rotate_slots(hc_ctx *c, bool piped, int n_out, Slot **slot)
{
  if (piped) {
    const int use = pipeline_slots(c->watch.pipe_slots, c->watch.big_slots, n_out, c->W, c->H);
    if (use != c->nslot_use) {
      if (int rc = finish_all(c)) return rc;
      c->nslot_use = use;
      c->cur = 0;
    }
  }
  Slot &s = c->slot[piped ? c->cur : 0];
  *slot = &s;
  if (!piped) { s.seq = 0; return finish_all(c); }
  if (int rc = alloc_slot(c, s)) return rc;
  if (int rc = finish_slot(c, s)) return rc;
  s.seq = ++c->run_seq;
  return HC_OK;
}

// Pipelined runs whose output [o0, o1) overlaps that of a run still in flight: that run is completed first -- should its
// queued launches not have reached the fixpoint, its host-side continuation rewrites whole maps (finish_slot) and would
// otherwise land on top of this run's result.  The same for an older run still in flight (a caller that alternates two
// output buffers): it is waited for, oldest first (once complete it patches nothing any more).
// *with_previous: the overlap is with the previous run (plan_front: no provisional map then)
int finish_overlapping(hc_ctx *c, uintptr_t o0, uintptr_t o1, bool *with_previous)
{
  *with_previous = false;
  for (int k = 1; k < c->nslot_use; ++k) {
    Slot &o = c->slot[(c->cur + k) % c->nslot_use];  // k = nslot_use - 1: the previous run
    if (!(o.out0 < o1 && o0 < o.out1)) continue;
    if (k == c->nslot_use - 1) *with_previous = true;
    if (int rc = finish_slot(c, o)) return rc;
  }
  return HC_OK;
}

// The front kernel of the planned form on stream sf.  fp: P.fp with the device pointers patched in.
int launch_front_form(hc_ctx *c, const FrontPlan &P, FrontParams &fp, const uint8_t *in_dy, hipStream_t sf)
{
  switch (P.form) {
  case HC_FORM_O_APERTURE5: case HC_FORM_O_GRADIENTS: case HC_FORM_O_APERTURE7: case HC_FORM_O_SCHARR: {
    FrontExtParams ep{};
    ep.f = fp;
    ep.gradients = in_dy ? 1 : 0;
    ep.channels = c->C;
    ep.dy = in_dy;
    ep.aperture = P.form == HC_FORM_O_APERTURE7 ? 7 : P.form == HC_FORM_O_SCHARR ? -1 : 5;
    HIPCK(launch_front_o_ext(ep, sf));
    break;
  }
  case HC_FORM_FRONT8O: HIPCK(launch_front8o(fp, sf)); break;
  case HC_FORM_FRONT_O: HIPCK(launch_front_o(fp, sf)); break;
  case HC_FORM_FRONT_MX: HIPCK(launch_front_mx(fp, sf)); break;
  case HC_FORM_FRONT8: case HC_FORM_FRONT8_HALF: HIPCK(launch_front8(fp, sf)); break;
#ifdef HC_LEGACY_FRONT
  case HC_FORM_SPLIT:  // k_blur + k_nms through the blur plane
    if (int rc = ensure_blur_plane(c)) return rc;
    fp.blur = c->d_bplane; fp.blur_frame_stride = c->bplane_fs;
    HIPCK(launch_blur(fp, sf));
    HIPCK(c->prof.mark(sf, P.mask_a, ProfRing::K_FRONT_A));
    HIPCK(launch_nms(fp, sf));
    break;
  case HC_FORM_FRONT4: HIPCK(launch_front(fp, sf)); break;
#endif
  default: return fail(HC_E_ARG, "internal: front kernel form");
  }
  return HC_OK;
}

// Final stages GAUSSIAN .. THRESH: the plain per-stage kernels up to `stage`, the last of them into dst, the others into
// the stage scratch planes.  mono: the one-channel frames (pitch mp, frame stride mfs)
int queue_stage_taps(hc_ctx *c, int stage, const uint8_t *mono, size_t mp, size_t mfs, uint8_t *dst, size_t dp, size_t dfs, int n, hipStream_t sf)
{
  const int W = c->W, H = c->H;
  ProfRing &prof = c->prof;
  if (int rc = ensure_stage_scratch(c)) return rc;
  const size_t bp = c->out_pitch, bfs = c->out_fs;  // scratch planes share the output geometry
  uint8_t *blur = stage == HC_STAGE_GAUSSIAN ? dst : c->d_blur;
  const size_t blp = stage == HC_STAGE_GAUSSIAN ? dp : bp, blfs = stage == HC_STAGE_GAUSSIAN ? dfs : bfs;
  // every plain kernel is booked on its own stage, as the reference's _endCudaTimer(stage) does (cannyEdgeH.cu:415-430)
  HIPCK(launch_gauss(mono, mp, mfs, blur, blp, blfs, W, H, n, sf));
  HIPCK(prof.mark(sf, B_GAUSS, ProfRing::K_FRONT_B));
  if (stage == HC_STAGE_GAUSSIAN) return HC_OK;
  HIPCK(launch_sobel(blur, blp, blfs, c->d_sx, c->d_sy, bp, bfs, W, H, n, sf));
  if (stage == HC_STAGE_GRADIENT) HIPCK(launch_graddisp(c->d_sx, c->d_sy, bp, bfs, dst, dp, dfs, W, H, n, sf));
  HIPCK(prof.mark(sf, B_GRAD, ProfRing::K_FRONT_B));
  if (stage == HC_STAGE_GRADIENT) return HC_OK;
  uint8_t *nms = stage == HC_STAGE_NMS ? dst : c->d_nms;
  const size_t np = stage == HC_STAGE_NMS ? dp : bp, nfs = stage == HC_STAGE_NMS ? dfs : bfs;
  HIPCK(launch_nms(c->d_sx, c->d_sy, bp, bfs, nms, np, nfs, W, H, n, c->opt.nms_saturate, sf));
  HIPCK(prof.mark(sf, B_NMS, ProfRing::K_FRONT_B));
  if (stage == HC_STAGE_NMS) return HC_OK;
  HIPCK(launch_thresh(nms, np, nfs, dst, dp, dfs, W, H, n, c->opt.low, c->opt.high, sf));
  HIPCK(prof.mark(sf, B_THR, ProfRing::K_FRONT_B));
  return HC_OK;
}

// in_dy != null: `in` and `in_dy` are the int16 dx / dy planes of cv::Canny's (dx, dy) overload (Mode O, HC_STAGE_HYSTER,
// even addresses / pitch / frame stride: k_front_o_ext reads them as they are, nothing is staged)
// call_opt != null (hc_canny_device): the front path is planned with these choices instead of the context's
int run_impl(hc_ctx *c, const uint8_t *in, size_t in_pitch, size_t in_fs, uint8_t *out, size_t out_pitch, size_t out_fs, int n, int stage,
             const uint8_t *in_dy = nullptr, const FrontOpts *call_opt = nullptr)
{
  if (c->mode == HC_MODE_O && stage != HC_STAGE_HYSTER)
    return fail(HC_E_ARG, "mode O (cv::Canny) produces the final edge map only (cv::Canny has no intermediate outputs)");
  if (c->mode == HC_MODE_O && c->per_channel) return fail(HC_E_ARG, "HC_OPT_PER_CHANNEL applies to mode R contexts");
  if (c->per_channel && stage != HC_STAGE_HYSTER) return fail(HC_E_ARG, "per-channel mode only produces the final edge maps (HC_STAGE_HYSTER)");
  // a per-frame threshold table applies to the runs that go by the context's thresholds (hc_canny_device brings its own)
  const int32_t *frame_thr = (c->mode == HC_MODE_O && !call_opt) ? c->frame_thr : nullptr;
  if (frame_thr && n > c->frame_thr_n) return fail(HC_E_ARG, "the run has more frames than the table of hc_frame_thresholds_device holds");
  const int W = c->W, H = c->H;
  const int n_out = c->per_channel ? 3 * n : n;  // output frames (= bit-plane frames)
  const bool piped = c->pipeline && stage == HC_STAGE_HYSTER;
  // 1. the slot of this run; runs whose output this one would overwrite
  Slot *slot = nullptr;
  if (int rc = rotate_slots(c, piped, n_out, &slot)) return rc;
  Slot &s = *slot;
  FrontIn fi{ c->mode, c->C, W, H, c->RD, c->nstrips, c->per_channel, stage, n };
  fi.in = View{ (uintptr_t)in, in_pitch, in_fs }; fi.out = View{ (uintptr_t)out, out_pitch, out_fs }; fi.in_dy = (uintptr_t)in_dy;
  fi.own_in = View{ 0, c->in_pitch, c->in_fs }; fi.own_mono = View{ 0, c->mono_pitch, c->mono_fs }; fi.own_out = View{ 0, c->out_pitch, c->out_fs };
  fi.o = call_opt ? *call_opt : c->opt; fi.dump_region = c->dump_region; fi.piped = piped; fi.nslot_use = c->nslot_use; fi.front_one = c->watch.front_one; fi.wl_cap = s.wl_cap;
  const bool out_internal = out_view_staged(fi.out);
  uint8_t *dst = out_internal ? c->d_out : out;
  if (piped) {
    const uintptr_t o0 = (uintptr_t)dst, o1 = o0 + (size_t)n_out * (out_internal ? c->out_fs : out_fs);
    if (int rc = finish_overlapping(c, o0, o1, &fi.out_overlap)) return rc;
    s.out0 = o0; s.out1 = o1;
  }
  // 2. what this run does
  const FrontPlan P = plan_front(fi);
  c->last.in_staged = P.in_staged ? 1 : 0;
  c->last.out_staged = P.out_staged ? 1 : 0;
  c->last.front_form = P.form;
  if (P.error) return fail(HC_E_ARG, P.error);
  // streams: the front kernels always run on the context stream, in order with the caller's own work on it (whatever
  // it did to the input before this call, whatever it does to it afterwards); pipelined mode puts the rest on s_hyst.
  // (A separate front stream tied to the context stream by events cost a 50 us bubble per run: every cross-stream wait
  // is a round trip through the command processor.)
  hipStream_t sf = c->stream, sh = piped ? s.s_hyst : c->stream;
  // 3. staging, stage 0
  const size_t dp = P.dst.pitch, dfs = P.dst.fs;
  const uint8_t *src = P.in_staged ? c->d_in : in;
  if (P.in_staged)
    if (int rc = copy_frames_d2d(c, sf, c->d_in, c->in_pitch, c->in_fs, in, in_pitch, in_fs, (size_t)W * c->C, n)) return rc;
  ProfRing &prof = c->prof;
  HIPCK(prof.begin_run(sf));
  const uint8_t *mono = src;
  if (P.gray) {
    uint8_t *grey = stage == HC_STAGE_MONO ? dst : c->d_mono;
    HIPCK(launch_gray(src, P.src.pitch, P.src.fs, grey, stage == HC_STAGE_MONO ? dp : c->mono_pitch, stage == HC_STAGE_MONO ? dfs : c->mono_fs, W, H, n, sf));
    if (stage != HC_STAGE_MONO) mono = c->d_mono;
    HIPCK(prof.mark(sf, B_MONO, ProfRing::K_STAGE0));
  } else if (stage == HC_STAGE_MONO) {
    if (int rc = copy_frames_d2d(c, sf, dst, dp, dfs, src, P.src.pitch, P.src.fs, (size_t)W, n)) return rc;
    HIPCK(prof.mark(sf, B_MONO, ProfRing::K_STAGE0));
  }

  if (stage == HC_STAGE_HYSTER) {
    // 4. the front kernel of the planned form, with the device pointers patched in
    FrontParams fp = P.fp;
    fp.in = mono; fp.sbits = s.d_sbits; fp.cbits = s.d_cbits;
    fp.frame_thr = frame_thr;
    s.prov = P.prov;
    if (P.prov) fp.prov_out = dst;
    if (c->opt.debug_taps) {
      if (int rc = ensure_debug_buffers(c)) return rc;
      if (P.form != HC_FORM_SPLIT) fp.dbg_blur = c->dbg.blur;
    }
    if (form_zeroes_flags(P.form)) {  // the 8-px kernels and k_front_mx: flag words they zero, dump areas and page of zeros (alloc_dump)
      const size_t R = c->dump_region;
      fp.zero_words = s.d_flags;
      fp.dump = c->d_dump; fp.dump_c = c->d_dump + (fp.half ? R : 2048); fp.dump_p = c->d_dump + (fp.half ? 2 * R : 4096);
      fp.zeros = c->d_dump + (fp.half ? 3 * R : 16384);
    }
    if (P.waves) c->last.front_waves = P.waves;
    if (int rc = launch_front_form(c, P, fp, in_dy, sf)) return rc;
    HIPCK(prof.mark(sf, P.mask, ProfRing::K_FRONT_B));
    // 5. taps
    if (c->opt.debug_taps) {  // what the front kernels hand to the hysteresis (which updates the STRONG plane in place)
      const size_t bytes = sizeof(u32) * (size_t)c->RD * H * (size_t)n_out;
      HIPCK(hipMemcpyAsync(c->dbg.s, s.d_sbits, bytes, hipMemcpyDeviceToDevice, sf));
      HIPCK(hipMemcpyAsync(c->dbg.c, s.d_cbits, bytes, hipMemcpyDeviceToDevice, sf));
      c->dbg.frames = n_out;
      c->dbg.blur_split = P.form == HC_FORM_SPLIT;
      c->dbg.blur_valid = c->mode == HC_MODE_R;
    }
    // 6. events between the front kernel and the hysteresis
    if (piped) {
      HIPCK(hipEventRecord(s.ev_front, sf));
      const int k = (int)(s.seq & 7);
      if (!c->ring.f[k]) { HIPCK(hipEventCreate(&c->ring.f[k])); HIPCK(hipEventCreate(&c->ring.d[k])); }
      HIPCK(hipEventRecord(c->ring.f[k], sf));
      c->ring.seq[k] = 0;  // (valid once the chain's end is recorded too)
      HIPCK(hipStreamWaitEvent(sh, s.ev_front, 0));
    }
    // 7. the hysteresis
    if (int rc = queue_hyst_expand(c, s, sh, dst, dp, dfs, n_out, piped, P.zeroed_words)) return rc;
  } else if (stage > HC_STAGE_MONO) {
    if (int rc = queue_stage_taps(c, stage, mono, P.mono.pitch, P.mono.fs, dst, dp, dfs, n, sf)) return rc;
  }

  // 8. copy-out, end of the run
  if (out_internal)
    if (int rc = copy_out_staged(c, s, sh, out, out_pitch, out_fs, n_out, s.pending)) return rc;
  // the hysteresis (and the copy-out of an unaligned caller buffer) end the run; for the earlier stages the copy-out
  // belongs to the last stage that ran
  if (stage == HC_STAGE_HYSTER) HIPCK(prof.mark(sh, B_HYST, ProfRing::K_HYST));
  else if (out_internal) HIPCK(prof.mark(sh, 1u << stage, ProfRing::K_FRONT_B));
  prof.end_run();
  if (stage == HC_STAGE_HYSTER) HIPCK(hipEventRecord(s.ev_done, sh));
  if (piped) {
    HIPCK(hipEventRecord(c->ring.d[s.seq & 7], sh));
    c->ring.seq[s.seq & 7] = s.seq;
  }
  c->last.slot = piped ? c->cur : 0;
  if (piped) c->cur = (c->cur + 1) % c->nslot_use;
  c->last.run_n = n_out;
  return HC_OK;
}

}  // namespace

extern "C" {

const char *hc_last_error(void) { return g_err.c_str(); }
#ifdef HC_LEGACY_FRONT
const char *hc_version(void) { return "hipcanny 0.4 (gfx950) + round-1 front kernels (test build)"; }
#else
const char *hc_version(void) { return "hipcanny 0.4 (gfx950)"; }
#endif

void *hc_host_alloc(size_t bytes)
{
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    fail(HC_E_HIP, "hipHostMalloc failed");
    return nullptr;
  }
  return p;
}

void hc_host_free(void *p)
{
  if (p) (void)hipHostFree(p);
}

hc_ctx *hc_create(int device, int width, int height, int channels, int max_batch, int mode)
{
  if (width <= 0 || height <= 0 || (channels != 1 && channels != 3) || max_batch <= 0 || (mode != HC_MODE_R && mode != HC_MODE_O)) {
    fail(HC_E_ARG, "hc_create: bad width/height/channels/max_batch/mode");
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    fail(HC_E_NOGPU, "hc_create: no HIP device (this library has no CPU fallback)");
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) { fail(HC_E_HIP, "hipSetDevice failed"); return nullptr; }
  hc_ctx *c = new hc_ctx();
  c->device = device; c->W = width; c->H = height; c->C = channels; c->max_batch = max_batch; c->mode = mode;
  if (mode == HC_MODE_O) { c->opt.low = 50; c->opt.high = 150; }
  c->nstrips = (width + STRIP_W - 1) / STRIP_W;
  c->RD = plane_row_dwords(width);
  if (!c->RD) { fail(HC_E_ARG, "hc_create: width above 8184 is not supported"); delete c; return nullptr; }
  auto ok = [&](hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    fail(HC_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return false;
  };
  bool good = ok(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking), "hipStreamCreate");
  c->stream = c->own_stream;
  // (a BGR row is read in 12-byte groups of 4 pixels: keep room for the ragged last group)
  good = good && alloc_frames(&c->d_in, &c->in_pitch, &c->in_fs, round_up((size_t)width, 8) * channels, height, max_batch, (size_t)width * channels) == HC_OK;
  good = good && alloc_frames(&c->d_out, &c->out_pitch, &c->out_fs, (size_t)width, height, max_batch, (size_t)width) == HC_OK;
  if (good && channels == 3) good = alloc_frames(&c->d_mono, &c->mono_pitch, &c->mono_fs, (size_t)width, height, max_batch) == HC_OK;
  good = good && alloc_slot(c, c->slot[0]) == HC_OK;
  good = good && alloc_dump(c, half_pays(width)) == HC_OK;
  c->prof.evpool.assign((size_t)ProfRing::EV_RUNS * ProfRing::EV_PER_RUN, nullptr);
  c->prof.runprof.assign((size_t)ProfRing::EV_RUNS, ProfRing::RunProf{});
  for (size_t i = 0; good && i < c->prof.evpool.size(); ++i) good = ok(hipEventCreate(&c->prof.evpool[i]), "hipEventCreate");
  if (good) {
    // cannyEdgeH.cu:372-380: float coefficients K * (1 / 159.0f), computed in binary32 on the host
    float gk[25];
    static const int K[25] = { 2, 4, 5, 4, 2, 4, 9, 12, 9, 4, 5, 12, 15, 12, 5, 4, 9, 12, 9, 4, 2, 4, 5, 4, 2 };
    volatile float r = 1 / 159.0f;
    for (int i = 0; i < 25; ++i) { volatile float k = (float)K[i]; volatile float v = k * r; gk[i] = v; }
    good = ok(check_gauss_coeffs(gk), "Gaussian coefficient table differs from the kernels' literals");
  }
  if (!good) { hc_destroy(c); return nullptr; }
  return c;
}

void hc_destroy(hc_ctx *c)
{
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  for (void *q : { (void *)c->d_in, (void *)c->d_mono, (void *)c->d_out, (void *)c->d_blur, (void *)c->d_nms, (void *)c->d_sx, (void *)c->d_sy, (void *)c->d_bplane, (void *)c->d_dump }) (void)hipFree(q);
  for (DeviceScratch *q : { &c->hist256, &c->edge_items, &c->hough, &c->hough_tab, &c->seg_items, &c->seg_tab, &c->circles, &c->ccl_items, &c->morph_mid, &c->thin, &c->feat }) (void)hipFree(q->p);
  for (Slot &q : c->slot) free_slot(q);
  free_debug_buffers(c);
  for (auto &e : c->prof.evpool) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : { c->ev_up, c->ev_ready, c->ev_ready2, c->ev_down, c->ev_switch }) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ring.f) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ring.d) if (e) (void)hipEventDestroy(e);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

int hc_set_thresholds(hc_ctx *c, int low, int high)
{
  if (!c) return fail(HC_E_ARG, "null context");
  const int tmax = c->mode == HC_MODE_O ? 32767 : 255;  // Mode O thresholds apply to |dx|+|dy| (up to 2040)
  low = std::max(0, std::min(tmax, low));
  high = std::max(0, std::min(tmax, high));
  if (low > high) std::swap(low, high);
  c->opt.low = low; c->opt.high = high;
  return HC_OK;
}

// Only the pointer is kept: the front kernels of the following runs read the table on the context stream.
int hc_frame_thresholds_device(hc_ctx *c, const void *d_thr, int nframes)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (c->mode != HC_MODE_O) return fail(HC_E_ARG, "hc_frame_thresholds_device: mode O contexts only");
  if (!d_thr) { c->frame_thr = nullptr; c->frame_thr_n = 0; return HC_OK; }
  if ((uintptr_t)d_thr & 3u) return fail(HC_E_ARG, "hc_frame_thresholds_device: the table must be 4-byte aligned");
  if (nframes <= 0 || nframes > c->max_batch) return fail(HC_E_ARG, "hc_frame_thresholds_device: nframes out of range");
  c->frame_thr = (const int32_t *)d_thr; c->frame_thr_n = nframes;
  return HC_OK;
}

int hc_get_thresholds(const hc_ctx *c, int *low, int *high)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (low) *low = c->opt.low;
  if (high) *high = c->opt.high;
  return HC_OK;
}

namespace {
// The context stream changes: everything queued on the outgoing stream up to now -- an hc_upload above all, whose frames the
// next hc_run reads on the incoming stream, but the caller's own work there as well: an event cannot tell them apart -- comes
// first on the incoming one.  With the copy streams the upload itself sits on g_h2d, behind ev_ready and ahead of ev_up: the
// incoming stream waits for ev_up as the outgoing one does.  Events only: the host waits for nothing, and a stream with
// nothing queued is passed at once.  ev_switch is this function's alone (ev_ready belongs to hc_upload).
int switch_stream(hc_ctx *c, hipStream_t to)
{
  if (to == c->stream) return HC_OK;
  HIPCK(hipSetDevice(c->device));
  if (!c->ev_switch) HIPCK(hipEventCreateWithFlags(&c->ev_switch, hipEventDisableTiming));
  if (hipEventRecord(c->ev_switch, c->stream) == hipSuccess) HIPCK(hipStreamWaitEvent(to, c->ev_switch, 0));
  else (void)hipGetLastError();  // a caller's stream that no longer exists: there is nothing left to order against
  if (c->ev_up) HIPCK(hipStreamWaitEvent(to, c->ev_up, 0));  // (never recorded: no upload went through g_h2d, nothing to wait for)
  c->stream = to;
  return HC_OK;
}
}  // namespace

int hc_set_stream(hc_ctx *c, void *s)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (int rc = finish_all(c)) return rc;
  return switch_stream(c, (hipStream_t)s);  // 0 = the null stream itself (ordered with everything the caller queued on it)
}

int hc_use_own_stream(hc_ctx *c)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (int rc = finish_all(c)) return rc;
  return switch_stream(c, c->own_stream);
}

int hc_set_tuning(hc_ctx *c, int chunk_rows, int hyst_launches)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (chunk_rows < 0 || chunk_rows > 16384) return fail(HC_E_ARG, "chunk_rows must be 0 (auto) or 1..16384");
  if (hyst_launches < 0 || hyst_launches > MAX_HYST_LAUNCHES) return fail(HC_E_ARG, "hyst_launches out of range (0 = auto, 1..96)");
  if (int rc = finish_all(c)) return rc;
  c->opt.chunk = chunk_rows;
  c->hopt.launches_set = hyst_launches != 0;
  c->hopt.launches = hyst_launches ? hyst_launches : 6;
  return HC_OK;
}

int hc_set_option(hc_ctx *c, int option, int value)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (int rc = finish_all(c)) return rc;
  if (option == HC_OPT_NMS_SATURATE) c->opt.nms_saturate = value != 0;
  else if (option == HC_OPT_PER_CHANNEL) {
    if (c->C != 3) return fail(HC_E_ARG, "HC_OPT_PER_CHANNEL needs a 3-channel context");
    if ((value != 0) != (c->per_channel != 0)) {  // output-side buffers change size: 3 edge maps per input frame
      HIPCK(hipSetDevice(c->device));
      HIPCK(hipDeviceSynchronize());
      for (Slot &q : c->slot) free_slot(q);  // (the slots beyond the first are allocated again by the pipelined runs that need them)
      (void)hipFree(c->d_out);
      c->d_out = nullptr;
      c->per_channel = value != 0;
      free_debug_buffers(c);
      if (c->d_bplane) { (void)hipFree(c->d_bplane); c->d_bplane = nullptr; c->bplane_frames = 0; }
      if (alloc_frames(&c->d_out, &c->out_pitch, &c->out_fs, (size_t)c->W, c->H, c->max_batch * (c->per_channel ? 3 : 1), (size_t)c->W) != HC_OK) return HC_E_HIP;
      if (alloc_slot(c, c->slot[0]) != HC_OK) return HC_E_HIP;
    }
  } else if (option == HC_OPT_FRONT_SPLIT) {
    if (value < 0 || value > 2) return fail(HC_E_ARG, "HC_OPT_FRONT_SPLIT: 0 (k_front), 1 (k_blur + k_nms) or 2 (k_front8)");
#ifndef HC_LEGACY_FRONT
    if (value != 2 && c->mode == HC_MODE_R)
      return fail(HC_E_ARG, "HC_OPT_FRONT_SPLIT 1 / 0: the round-1 front kernels are not part of this library (parity tests load libhipcanny_legacy.so)");
#endif
    c->opt.split = value;
  } else if (option == HC_OPT_COPY_STREAMS) {
    if (c->dl.host) return fail(HC_E_STATE, "HC_OPT_COPY_STREAMS: a download is in flight");
    HIPCK(hipSetDevice(c->device));
    if (value && c->device < MAX_DEVICES) {
      std::lock_guard<std::mutex> lock(g_copy_streams_mutex);
      if (!g_h2d[c->device]) HIPCK(hipStreamCreateWithFlags(&g_h2d[c->device], hipStreamNonBlocking));
      if (!g_d2h[c->device]) HIPCK(hipStreamCreateWithFlags(&g_d2h[c->device], hipStreamNonBlocking));
      if (!c->ev_up) HIPCK(hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming));
      if (!c->ev_ready) HIPCK(hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming));
      if (!c->ev_ready2) HIPCK(hipEventCreateWithFlags(&c->ev_ready2, hipEventDisableTiming));
      if (!c->ev_down) HIPCK(hipEventCreateWithFlags(&c->ev_down, hipEventDisableTiming));
    }
    c->copy_streams = value != 0 && c->device < MAX_DEVICES;
  } else if (option == HC_OPT_FRONT_WPB) {
    if (value != -1 && value != 1 && value != 4) return fail(HC_E_ARG, "HC_OPT_FRONT_WPB: -1 (automatic), 1 or 4");
    c->opt.wpb_mode = value;
  } else if (option == HC_OPT_PIPELINE_SLOTS) {
    if (value == -1 || value == 20 || value == 21) { c->watch.pipe_slots = 0; c->watch.chain_told = value == 20 ? 1 : value == 21 ? -1 : 0; }
    else if (value == 2 || value == 3) c->watch.pipe_slots = value;
    else return fail(HC_E_ARG, "HC_OPT_PIPELINE_SLOTS: -1 (automatic), 2, 3, or 20 / 21 (diagnostics)");
  } else if (option == HC_OPT_FRONT_DENSE) {
    if (value < -1 || value > 1) return fail(HC_E_ARG, "HC_OPT_FRONT_DENSE: -1 (automatic), 0 (never) or 1 (every window)");
    c->opt.dense_mode = value;
  } else if (option == HC_OPT_FRONT_MX) {
    if (value != 0 && value != 1) return fail(HC_E_ARG, "HC_OPT_FRONT_MX: 0 (never) or 1 (whenever the run allows it)");
    c->opt.mx_mode = value;
  } else if (option == HC_OPT_TEST_HYST_LATE_GRID) {  // tests: tiny grids exercise the hand-on of worklist entries
    c->hopt.late_grid = std::max(-1, value);
  } else if (option == HC_OPT_TEST_HYST_LOOP) {
    c->hopt.loop = value != 0;
  } else if (option == HC_OPT_TEST_HYST_DIAG) {
    c->hopt.diag = value != 0;
  } else if (option == HC_OPT_TEST_HYST_GEOM) {  // rows per wave x 100 + waves per workgroup; 0: by the rule
    c->hopt.geom = std::max(0, value);
  } else if (option == HC_OPT_TEST_DENSE_ENTER) {
    c->opt.dense_enter = std::max(0, value);
  } else if (option == HC_OPT_TEST_DENSE_LEAVE) {
    c->opt.dense_leave = std::max(0, value);
  } else if (option == HC_OPT_TEST_HOUGH_SCRATCH) {  // tests: a small bound cuts a small batch into several passes; <= 0: the default
    c->hough_bound = value > 0 ? (size_t)value : HOUGH_SCRATCH_BYTES;
  } else if (option == HC_OPT_TEST_HOUGH_ROWS) {  // measurements: the angles per workgroup of k_hough_vote (capped by LDS, HOUGH_MAX_ROWS and numangle); <= 0: by the rule
    c->hough_rows = std::max(0, value);
  } else if (option == HC_OPT_FRONT_HALF) {
    if (value < -1 || value > 1) return fail(HC_E_ARG, "HC_OPT_FRONT_HALF: -1 (automatic), 0 (never) or 1 (whenever possible)");
    HIPCK(hipSetDevice(c->device));
    if (value == 1 && !c->dump_region) {  // the half-strip form needs the larger dump areas
      HIPCK(hipDeviceSynchronize());
      if (int rc = alloc_dump(c, true)) return rc;
    }
    c->opt.half_mode = value;
  } else if (option == HC_OPT_L2_GRADIENT) {
    if (c->mode != HC_MODE_O) return fail(HC_E_ARG, "HC_OPT_L2_GRADIENT applies to mode O contexts");
    c->opt.l2gradient = value != 0;
  } else if (option == HC_OPT_APERTURE) {
    if (c->mode != HC_MODE_O) return fail(HC_E_ARG, "HC_OPT_APERTURE applies to mode O contexts");
    if (value == 7)
      return fail(HC_E_ARG, "HC_OPT_APERTURE 7 is not offered: cv::Canny scales the 7x7 Sobel and its thresholds to stay within "
                            "int16, which HC_OPT_APERTURE does not restate; hc_canny_device takes the aperture (7, and -1 for Scharr) and "
                            "cv::Canny's own thresholds per call; hc_derivatives_device computes those derivatives for hc_run_gradients_device");
    if (value != 3 && value != 5) return fail(HC_E_ARG, "HC_OPT_APERTURE: 3 (default) or 5");
    c->opt.aperture = value;
  } else if (option == HC_OPT_DEBUG_TAPS) {
    c->opt.debug_taps = value != 0;
    c->dbg.frames = 0;
  } else if (option == HC_OPT_PIPELINE) {
    HIPCK(hipSetDevice(c->device));
    if (value && alloc_slot(c, c->slot[1]) != HC_OK) return HC_E_HIP;  // (the slots of the four-slot ring are allocated by the small batches that use them)
    c->pipeline = value != 0;
    c->cur = 0;
    c->nslot_use = 2;
  } else return fail(HC_E_ARG, "hc_set_option: unknown option");
  return HC_OK;
}

int hc_upload(hc_ctx *c, const uint8_t *host, size_t row_stride, size_t frame_stride, int n)
{
  if (!c || !host) return fail(HC_E_ARG, "hc_upload: null argument");
  if (n <= 0 || n > c->max_batch) return fail(HC_E_ARG, "hc_upload: nframes out of range");
  const size_t rb = (size_t)c->W * c->C;
  if (int rc = check_host_rows("hc_upload", row_stride, rb)) return rc;
  HIPCK(hipSetDevice(c->device));
  if (int rc = finish_all(c)) return rc;
  // cannyEdgeH.cu:136/144 (cudaMemcpy2D host -> pitched device).  Tight rows on both sides: one contiguous block, one DMA
  hipStream_t cs = c->copy_streams ? g_h2d[c->device] : c->stream;
  if (c->copy_streams && hipStreamQuery(c->stream) != hipSuccess) {  // what is still queued on the context stream (it may read d_in) comes first
    HIPCK(hipEventRecord(c->ev_ready, c->stream));
    HIPCK(hipStreamWaitEvent(cs, c->ev_ready, 0));
  }
  if (row_stride == rb && c->in_pitch == rb && frame_stride == c->in_fs)
    HIPCK(hipMemcpyAsync(c->d_in, host, c->in_fs * (size_t)n, hipMemcpyHostToDevice, cs));
  else
    for (int f = 0; f < n; ++f)
      HIPCK(hipMemcpy2DAsync(c->d_in + c->in_fs * f, c->in_pitch, host + frame_stride * f, row_stride, rb, (size_t)c->H, hipMemcpyHostToDevice, cs));
  if (c->copy_streams) {
    HIPCK(hipEventRecord(c->ev_up, cs));
    HIPCK(hipStreamWaitEvent(c->stream, c->ev_up, 0));
  }
  c->uploaded = n;
  return HC_OK;
}

int hc_run(hc_ctx *c, int final_stage, int n)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (final_stage < HC_STAGE_MONO || final_stage > HC_STAGE_HYSTER) return fail(HC_E_ARG, "Canny Stage Not Recognized");
  if (n <= 0 || n > c->uploaded) return fail(HC_E_STATE, "hc_run: more frames than uploaded");
  if (c->dl.host) return fail(HC_E_STATE, "hc_run: a download of the internal output buffer is in flight (hc_download_end first)");
  HIPCK(hipSetDevice(c->device));
  return run_impl(c, c->d_in, c->in_pitch, c->in_fs, c->d_out, c->out_pitch, c->out_fs, n, final_stage);
}

int hc_run_device(hc_ctx *c, const void *d_in, size_t in_pitch, size_t in_fs, void *d_out, size_t out_pitch, size_t out_fs, int n, int final_stage)
{
  if (!c || !d_in || !d_out) return fail(HC_E_ARG, "hc_run_device: null argument");
  if (final_stage < HC_STAGE_MONO || final_stage > HC_STAGE_HYSTER) return fail(HC_E_ARG, "Canny Stage Not Recognized");
  if (int rc = check_views(c, "hc_run_device", n, c->max_batch, { { "d_in (in_pitch, in_fs)", d_in, in_pitch, in_fs, (size_t)c->W * c->C }, { "d_out (out_pitch, out_fs)", d_out, out_pitch, out_fs, (size_t)c->W } })) return rc;
  HIPCK(hipSetDevice(c->device));
  return run_impl(c, (const uint8_t *)d_in, in_pitch, in_fs, (uint8_t *)d_out, out_pitch, out_fs, n, final_stage);
}

int hc_run_gradients_device(hc_ctx *c, const void *d_dx, const void *d_dy, size_t pitch, size_t frame_stride, void *d_out, size_t out_pitch,
                            size_t out_frame_stride, int n)
{
  if (!c || !d_dx || !d_dy || !d_out) return fail(HC_E_ARG, "hc_run_gradients_device: null argument");
  if (c->mode != HC_MODE_O) return fail(HC_E_ARG, "hc_run_gradients_device: mode O contexts only (cv::Canny's (dx, dy) overload)");
  const size_t row16 = (size_t)2 * c->C * c->W;
  if (int rc = check_views(c, "hc_run_gradients_device", n, c->max_batch, { { "d_dx (pitch, frame_stride)", d_dx, pitch, frame_stride, row16, 2 }, { "d_dy (pitch, frame_stride)", d_dy, pitch, frame_stride, row16, 2 },
                                                                            { "d_out (out_pitch, out_frame_stride)", d_out, out_pitch, out_frame_stride, (size_t)c->W } })) return rc;
  HIPCK(hipSetDevice(c->device));
  return run_impl(c, (const uint8_t *)d_dx, pitch, frame_stride, (uint8_t *)d_out, out_pitch, out_frame_stride, n, HC_STAGE_HYSTER,
                  (const uint8_t *)d_dy);
}

int hc_canny_device(hc_ctx *c, const void *d_in, size_t in_pitch, size_t in_fs, void *d_out, size_t out_pitch, size_t out_fs, int n, double low,
                    double high, int aperture, int l2gradient)
{
  if (!c || !d_in || !d_out) return fail(HC_E_ARG, "hc_canny_device: null argument");
  if (c->mode != HC_MODE_O) return fail(HC_E_ARG, "hc_canny_device: mode O contexts only (cv::Canny)");
  if (!deriv_ksize_ok(aperture)) return fail(HC_E_ARG, "hc_canny_device: aperture 3, 5, 7 or -1 (Scharr)");
  CallThresholds t;
  if (!canny_call_thresholds(low, high, aperture, l2gradient != 0, &t)) return fail(HC_E_ARG, "hc_canny_device: thresholds must be finite and not negative");
  if (int rc = check_views(c, "hc_canny_device", n, c->max_batch, { { "d_in (in_pitch, in_fs)", d_in, in_pitch, in_fs, (size_t)c->W * c->C }, { "d_out (out_pitch, out_fs)", d_out, out_pitch, out_fs, (size_t)c->W } })) return rc;
  HIPCK(hipSetDevice(c->device));
  // the call's own choices, on a copy: the context's thresholds, HC_OPT_APERTURE and HC_OPT_L2_GRADIENT stay as they are
  FrontOpts o = c->opt;
  o.aperture = aperture; o.l2gradient = l2gradient != 0; o.call_lo = t.k_lo; o.call_hi = t.k_hi;
  return run_impl(c, (const uint8_t *)d_in, in_pitch, in_fs, (uint8_t *)d_out, out_pitch, out_fs, n, HC_STAGE_HYSTER, nullptr, &o);
}

// Not a run: one kernel on the context stream, in order with whatever is queued there (a following hc_run_gradients_device
// reads the planes through its front kernel on the same stream).  Touches no slot, plan, timer or diagnostic of the runs.
int hc_derivatives_device(hc_ctx *c, const void *d_in, size_t in_pitch, size_t in_fs, void *d_dx, void *d_dy, size_t pitch, size_t fs, int n,
                          int ksize)
{
  if (!c || !d_in || !d_dx || !d_dy) return fail(HC_E_ARG, "hc_derivatives_device: null argument");
  if (!deriv_ksize_ok(ksize)) return fail(HC_E_ARG, "hc_derivatives_device: ksize 3, 5, 7 (scaled by 1/16, as in cv::Canny) or -1 (Scharr)");
  const size_t row = (size_t)c->C * c->W;
  if (int rc = check_views(c, "hc_derivatives_device", n, c->max_batch, { { "d_in (in_pitch, in_fs)", d_in, in_pitch, in_fs, row, 1, true }, { "d_dx (pitch, fs)", d_dx, pitch, fs, 2 * row, 2, true },
                                                                          { "d_dy (pitch, fs)", d_dy, pitch, fs, 2 * row, 2, true } })) return rc;
  const DerivPlan P = plan_derivatives(c->W, c->H, c->C, View{ (uintptr_t)d_in, in_pitch, in_fs }, View{ (uintptr_t)d_dx, pitch, fs }, (uintptr_t)d_dy, n, ksize);
  if (P.error) return fail(HC_E_ARG, std::string("hc_derivatives_device: ") + P.error);
  HIPCK(hipSetDevice(c->device));
  HIPCK(launch_deriv16(P.dp, c->stream));
  return HC_OK;
}

// host only: the rule is stated in include/hipcanny.h, the arithmetic is gaussian_taps_q8 (host_plan.h)
int hc_gaussian_taps_q8(int ksize, double sigma, uint16_t *taps)
{
  if (!taps) return fail(HC_E_ARG, "hc_gaussian_taps_q8: null argument");
  if (!blur_ksize_ok(ksize)) return fail(HC_E_ARG, "hc_gaussian_taps_q8: ksize 3, 5 or 7");
  if (!gaussian_taps_q8(ksize, sigma, taps)) return fail(HC_E_ARG, "hc_gaussian_taps_q8: sigma must be finite and give taps of 0 .. 256");
  return HC_OK;
}

// host only: the rule is stated in include/hipcanny.h, the arithmetic is structuring_spans (host_plan.h)
int hc_structuring_element(int shape, int ksize, int8_t *spans)
{
  if (!spans) return fail(HC_E_ARG, "hc_structuring_element: null argument");
  if (!blur_ksize_ok(ksize)) return fail(HC_E_ARG, "hc_structuring_element: ksize 3, 5 or 7");
  if (!structuring_spans(shape, ksize, spans)) return fail(HC_E_ARG, "hc_structuring_element: shape must be HC_MORPH_RECT, HC_MORPH_CROSS or HC_MORPH_ELLIPSE");
  return HC_OK;
}

// host only: geometry and tables of hc_hough_lines_device by the rule include/hipcanny.h states (hough_tables, host_plan.h)
int hc_hough_tables(int width, int height, double rho, double theta, double min_theta, double max_theta, int *numangle, int *numrho, float *tab_cos,
                    float *tab_sin, float *tab_theta, size_t table_capacity)
{
  if (const char *e = hough_tables(width, height, rho, theta, min_theta, max_theta, numangle, numrho, tab_cos, tab_sin, tab_theta, table_capacity))
    return fail(HC_E_ARG, std::string("hc_hough_tables: ") + e);
  return HC_OK;
}

// host only: the walk tables of hc_hough_segments_device by the rule include/hipcanny.h states (hough_walk_tables, host_plan.h)
int hc_hough_walk_tables(int width, int height, double rho, double theta, double min_theta, double max_theta, int *numangle, int32_t *major, float *slope,
                         float *scale, size_t table_capacity)
{
  if (const char *e = hough_walk_tables(width, height, rho, theta, min_theta, max_theta, numangle, major, slope, scale, table_capacity))
    return fail(HC_E_ARG, std::string("hc_hough_walk_tables: ") + e);
  return HC_OK;
}

// host only: the accumulator and the smallest squared distance of hc_hough_circles_device (hough_circle_geometry, host_plan.h)
int hc_hough_circle_geometry(int width, int height, double dp, double min_dist, int min_radius, int max_radius, int *acc_width, int *acc_height, long long *min_d2)
{
  if (const char *e = hough_circle_geometry(width, height, dp, min_dist, min_radius, max_radius, acc_width, acc_height, min_d2))
    return fail(HC_E_ARG, std::string("hc_hough_circle_geometry: ") + e);
  return HC_OK;
}

int hc_hysteresis_device(hc_ctx *c, const void *d_thresh, size_t in_pitch, size_t in_fs, void *d_out, size_t out_pitch, size_t out_fs, int n)
{
  if (!c || !d_thresh || !d_out) return fail(HC_E_ARG, "hc_hysteresis_device: null argument");
  if (int rc = check_views(c, "hc_hysteresis_device", n, c->max_batch, { { "d_thresh (in_pitch, in_fs)", d_thresh, in_pitch, in_fs, (size_t)c->W }, { "d_out (out_pitch, out_fs)", d_out, out_pitch, out_fs, (size_t)c->W } })) return rc;
  HIPCK(hipSetDevice(c->device));
  if (int rc = finish_all(c)) return rc;
  Slot &s = c->slot[0];
  PackParams pp{};
  pp.in = (const uint8_t *)d_thresh; pp.in_pitch = in_pitch; pp.in_frame_stride = in_fs; pp.sbits = s.d_sbits; pp.cbits = s.d_cbits; pp.RD = c->RD; pp.W = c->W; pp.H = c->H; pp.nframes = n;
  HIPCK(launch_pack(pp, c->stream));
  const View out{ (uintptr_t)d_out, out_pitch, out_fs };
  const bool out_internal = out_view_staged(out);
  const View dst = out_internal ? View{ (uintptr_t)c->d_out, c->out_pitch, c->out_fs } : out;
  s.prov = false;  // nothing has written a provisional map into this output (a pipelined run may have left the flag set)
  if (int rc = queue_hyst_expand(c, s, c->stream, (uint8_t *)dst.p, dst.pitch, dst.fs, n, false)) return rc;
  if (out_internal)
    if (int rc = copy_out_staged(c, s, c->stream, d_out, out_pitch, out_fs, n, true)) return rc;
  HIPCK(hipEventRecord(s.ev_done, c->stream));
  return HC_OK;
}

int hc_sync(hc_ctx *c)
{
  if (!c) return fail(HC_E_ARG, "null context");
  HIPCK(hipSetDevice(c->device));
  if (int rc = finish_all(c)) return rc;
  for (Slot &q : c->slot)
    if (q.s_hyst) HIPCK(hipStreamSynchronize(q.s_hyst));
  HIPCK(hipStreamSynchronize(c->stream));
  if (int rc = c->prof.collect()) return rc;
  return HC_OK;
}

int hc_download(hc_ctx *c, uint8_t *host, size_t row_stride, size_t frame_stride, int n)
{
  if (!c || !host) return fail(HC_E_ARG, "hc_download: null argument");
  if (n <= 0 || n > c->last.run_n) return fail(HC_E_STATE, "hc_download: more frames than the last run produced");
  if (int rc = check_host_rows("hc_download", row_stride, (size_t)c->W)) return rc;
  if (int rc = hc_sync(c)) return rc;
  if (int rc = copy_out_d2h(c, host, row_stride, frame_stride, n, c->stream)) return rc;
  HIPCK(hipStreamSynchronize(c->stream));
  return HC_OK;
}

namespace {
int queue_download(hc_ctx *c)
{
  hipStream_t cs = c->copy_streams ? g_d2h[c->device] : c->stream;
  if (c->copy_streams) {  // behind everything queued on the context stream (the run, its copy-out kernels)
    HIPCK(hipEventRecord(c->ev_ready2, c->stream));
    HIPCK(hipStreamWaitEvent(cs, c->ev_ready2, 0));
    Slot &s = c->slot[c->last.slot];
    // Redundant, kept as a second line of defence: hc_download_begin has already made the context stream wait for this
    // ev_done, ahead of the ev_ready2 recorded above, and on the repeated copy (hc_download_end) finish_all has completed
    // the run.  Removing it alone changes no result; tests/test_gpu_host_fed.py pins hc_download_begin's wait.
    if (s.pending && s.stream != c->stream) HIPCK(hipStreamWaitEvent(cs, s.ev_done, 0));
  }
  if (int rc = copy_out_d2h(c, c->dl.host, c->dl.row, c->dl.fs, c->dl.n, cs)) return rc;
  if (c->copy_streams) HIPCK(hipEventRecord(c->ev_down, cs));
  return HC_OK;
}
}  // namespace

int hc_download_begin(hc_ctx *c, uint8_t *host, size_t row_stride, size_t frame_stride, int n)
{
  if (!c || !host) return fail(HC_E_ARG, "hc_download_begin: null argument");
  if (n <= 0 || n > c->last.run_n) return fail(HC_E_STATE, "hc_download_begin: more frames than the last run produced");
  if (int rc = check_host_rows("hc_download_begin", row_stride, (size_t)c->W)) return rc;
  if (c->dl.host) return fail(HC_E_STATE, "hc_download_begin: a download is already in flight (hc_download_end first)");
  HIPCK(hipSetDevice(c->device));
  // behind the run: its hysteresis may sit on the slot's own stream (pipelined mode)
  Slot &s = c->slot[c->last.slot];
  if (s.pending && s.stream != c->stream) HIPCK(hipStreamWaitEvent(c->stream, s.ev_done, 0));
  c->dl.host = host; c->dl.row = row_stride; c->dl.fs = frame_stride; c->dl.n = n;
  c->dl.stale = false;
  if (int rc = queue_download(c)) { c->dl.host = nullptr; return rc; }
  return HC_OK;
}

int hc_download_end(hc_ctx *c)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (!c->dl.host) return fail(HC_E_STATE, "hc_download_end without hc_download_begin");
  HIPCK(hipSetDevice(c->device));
  int rc = finish_all(c);  // convergence of every run in flight; the host-side continuation if one needed it
  // the maps changed after the copy was queued -- here, or in any entry point that finished the runs since hc_download_begin
  // (hc_upload, hc_sync, hc_set_option, hc_hysteresis_totals ...): copy them again
  if (rc == HC_OK && c->dl.stale) rc = queue_download(c);
  c->dl.stale = false;
  if (rc == HC_OK && (c->copy_streams ? hipEventSynchronize(c->ev_down) : hipStreamSynchronize(c->stream)) != hipSuccess) rc = fail(HC_E_HIP, "waiting for the download failed");
  c->dl.host = nullptr;
  return rc;
}

int hc_enable_profiling(hc_ctx *c, int on)
{
  if (!c) return fail(HC_E_ARG, "null context");
  c->prof.on = on != 0;
  return HC_OK;
}

int hc_profile_get(hc_ctx *c, double sum_ms[3], long *nruns, int reset)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (int rc = hc_sync(c)) return rc;
  if (sum_ms) for (int i = 0; i < 3; ++i) sum_ms[i] = c->prof.sum[i];
  if (nruns) *nruns = c->prof.runs;
  if (reset) {
    c->prof.step_ms.clear(); c->prof.prev_end = nullptr;
    c->prof.front_each.clear();
    c->prof.sum[0] = c->prof.sum[1] = c->prof.sum[2] = 0; c->prof.runs = 0;
    c->prof.split_sum[0] = c->prof.split_sum[1] = 0; c->prof.split_runs = 0;
  }
  return HC_OK;
}

int hc_profile_get_front(hc_ctx *c, double sum_ms[2], long *nruns)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (int rc = hc_sync(c)) return rc;
  if (sum_ms) { sum_ms[0] = c->prof.split_sum[0]; sum_ms[1] = c->prof.split_sum[1]; }
  if (nruns) *nruns = c->prof.split_runs;
  return HC_OK;
}

int hc_profile_get_intervals(hc_ctx *c, float *ms, int cap, int *n)
{
  if (!c || !n || (cap > 0 && !ms)) return fail(HC_E_ARG, "hc_profile_get_intervals: bad argument");
  if (int rc = hc_sync(c)) return rc;
  const int m = (int)std::min<size_t>(c->prof.step_ms.size(), (size_t)std::max(cap, 0));
  for (int i = 0; i < m; ++i) ms[i] = c->prof.step_ms[(size_t)i];
  *n = (int)c->prof.step_ms.size();
  return HC_OK;
}

int hc_profile_get_front_each(hc_ctx *c, float *ms, int cap, int *n)
{
  if (!c || !n || (cap > 0 && !ms)) return fail(HC_E_ARG, "hc_profile_get_front_each: bad argument");
  if (int rc = hc_sync(c)) return rc;
  const int m = (int)std::min<size_t>(c->prof.front_each.size(), (size_t)std::max(cap, 0));
  for (int i = 0; i < m; ++i) ms[i] = c->prof.front_each[(size_t)i];
  *n = (int)c->prof.front_each.size();
  return HC_OK;
}

int hc_stage_time_ms(hc_ctx *c, int stage, float *ms)
{
  if (!c || !ms || stage < 0 || stage > 5) return fail(HC_E_ARG, "hc_stage_time_ms: bad argument");
  *ms = (c->prof.stage_ran >> stage & 1u) ? c->prof.stage_ms[stage] : -1.0f;
  return HC_OK;
}

int hc_device_ptrs(hc_ctx *c, void **d_in, void **d_out, size_t *in_pitch, size_t *out_pitch, size_t *in_fs, size_t *out_fs)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (d_in) *d_in = c->d_in;
  if (d_out) *d_out = c->d_out;
  if (in_pitch) *in_pitch = c->in_pitch;
  if (out_pitch) *out_pitch = c->out_pitch;
  if (in_fs) *in_fs = c->in_fs;
  if (out_fs) *out_fs = c->out_fs;
  return HC_OK;
}

int hc_debug_tap(hc_ctx *c, int what, uint8_t *host, size_t row_stride, size_t frame_stride, int n)
{
  if (!c || !host) return fail(HC_E_ARG, "hc_debug_tap: null argument");
  if (what != HC_TAP_BLUR && what != HC_TAP_THRESH) return fail(HC_E_ARG, "hc_debug_tap: unknown tap");
  if (int rc = check_host_rows("hc_debug_tap", row_stride, (size_t)c->W)) return rc;
  if (int rc = hc_sync(c)) return rc;
  if (!c->opt.debug_taps || n <= 0 || n > c->dbg.frames) return fail(HC_E_STATE, "hc_debug_tap: set HC_OPT_DEBUG_TAPS and run HC_STAGE_HYSTER first");
  const int W = c->W, H = c->H;
  if (what == HC_TAP_THRESH) {
    const size_t words = (size_t)c->RD * H * (size_t)n;
    std::vector<u32> sb(words), cb(words);
    HIPCK(hipMemcpy(sb.data(), c->dbg.s, words * 4, hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(cb.data(), c->dbg.c, words * 4, hipMemcpyDeviceToHost));
    for (int f = 0; f < n; ++f)
      for (int r = 0; r < H; ++r) {
        const u32 *srow = &sb[((size_t)f * H + r) * c->RD], *crow = &cb[((size_t)f * H + r) * c->RD];
        uint8_t *o = host + frame_stride * f + row_stride * r;
        for (int x = 0; x < W; ++x) {
          const u32 sbit = (srow[x >> 5] >> (x & 31)) & 1u, cbit = (crow[x >> 5] >> (x & 31)) & 1u;
          o[x] = sbit ? 255 : cbit ? 128 : 0;
        }
      }
    return HC_OK;
  }
  if (!c->dbg.blur_valid) return fail(HC_E_STATE, "hc_debug_tap: the last run computed no blur (mode O)");
  if (c->dbg.blur_split) {  // [frame][strip][H][256]: bytes 4..251 of a segment row are the strip's 248 columns
    std::vector<uint8_t> seg((size_t)H * 256);
    for (int f = 0; f < n; ++f)
      for (int st = 0; st < c->nstrips; ++st) {
        HIPCK(hipMemcpy(seg.data(), c->d_bplane + c->bplane_fs * f + (size_t)st * H * 256, seg.size(), hipMemcpyDeviceToHost));
        const int x0 = st * STRIP_W, nx = std::min(STRIP_W, W - x0);
        for (int r = 0; r < H; ++r) std::memcpy(host + frame_stride * f + row_stride * r + x0, &seg[(size_t)r * 256 + 4], (size_t)nx);
      }
  } else {
    for (int f = 0; f < n; ++f)
      HIPCK(hipMemcpy2D(host + frame_stride * f, row_stride, c->dbg.blur + c->out_fs * f, c->out_pitch, (size_t)W, (size_t)H, hipMemcpyDeviceToHost));
  }
  return HC_OK;
}

int hc_pipeline_depth(hc_ctx *c, int nframes)
{
  if (!c || nframes <= 0) return fail(HC_E_ARG, "hc_pipeline_depth: null context or nframes <= 0");
  return pipeline_depth(c->pipeline, c->watch.pipe_slots, c->watch.big_slots, c->per_channel ? 3 * nframes : nframes, c->W, c->H);
}

int hc_front_waves_per_workgroup(hc_ctx *c)
{
  if (!c) return fail(HC_E_ARG, "null context");
  return c->last.front_waves;
}

int hc_pipeline_slots_in_use(hc_ctx *c)
{
  if (!c) return fail(HC_E_ARG, "null context");
  return c->pipeline ? c->nslot_use : 1;
}

int hc_last_run_info(hc_ctx *c, int *input_staged, int *output_staged, int *front_form)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (input_staged) *input_staged = c->last.in_staged;
  if (output_staged) *output_staged = c->last.out_staged;
  if (front_form) *front_form = c->last.front_form;
  return HC_OK;
}

int hc_hysteresis_stats(hc_ctx *c, unsigned *stats, int nwords)
{
  if (!c || !stats) return fail(HC_E_ARG, "null argument");
  if (int rc = finish_all(c)) return rc;
  for (int i = 0; i < nwords && i < 3 * MAX_HYST_LAUNCHES; ++i) stats[i] = c->last.stats[i];
  return HC_OK;
}

int hc_last_hysteresis_info(hc_ctx *c, int *launches_with_work, int *continued)
{
  if (!c) return fail(HC_E_ARG, "null context");
  if (int rc = finish_all(c)) return rc;
  if (launches_with_work) *launches_with_work = c->hist.last_work_launches;
  if (continued) *continued = c->last.continued;
  return HC_OK;
}

int hc_last_hysteresis_schedule(hc_ctx *c, int *info, int nwords)
{
  if (!c || !info) return fail(HC_E_ARG, "null argument");
  if (int rc = finish_all(c)) return rc;
  for (int i = 0; i < nwords && i < HC_SCHED_WORDS; ++i) info[i] = c->last.sched[i];
  return HC_OK;
}

int hc_hysteresis_totals(hc_ctx *c, unsigned long long totals[4], int reset)
{
  if (!c || !totals) return fail(HC_E_ARG, "null argument");
  if (int rc = finish_all(c)) return rc;
  for (int i = 0; i < 4; ++i) totals[i] = c->last.totals[i];
  if (reset) for (int i = 0; i < 4; ++i) c->last.totals[i] = 0;
  return HC_OK;
}

int hc_selftest(int device)
{
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(HC_E_NOGPU, "hc_selftest: no HIP device");
  HIPCK(hipSetDevice(device));
  u32 *d = nullptr, h = 0xFFFFFFFFu;
  HIPCK(hipMalloc((void **)&d, sizeof(u32)));
  HIPCK(hipMemset(d, 0, sizeof(u32)));
  HIPCK(launch_selftest(d, nullptr));
  HIPCK(hipMemcpy(&h, d, sizeof(u32), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  if (h) return fail(HC_E_HIP, "hc_selftest: primitive check failed, bits=" + std::to_string(h));
  return HC_OK;
}
}  // extern "C"
