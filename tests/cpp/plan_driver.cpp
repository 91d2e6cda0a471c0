// plan_driver.cpp -- the planner of cudacam_amd/csrc/host_plan.h, checked without a GPU (tests/test_plan_cpu.py builds this
// with g++ under ASan + UBSan).  A context is modelled with the same helpers hc_create uses (frame_pitch,
// plane_row_dwords, half_pays, half_dump_region, slot_wl_cap); every plan of the sweep must keep the capacity claims the
// launchers and kernels rest on.  Every front plan the driver makes is also folded into a 64-bit FNV-1a digest, field by field:
// tests/golden/plan_front_digest.json holds the value of the commit named there, so a restructured planner proves that it
// plans what that one planned.  check_view (every entry point's view rules) and the plans of the entries that are not runs
// (plan_derivatives, plan_histogram, plan_edge_points) are checked beside them, outside the count and the digest.
// Prints "ok <plans checked> <digest>" or the first violations.
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace hc;

static long g_plans = 0, g_fail = 0;
static void bad(const char *what, const FrontIn &in, const FrontPlan &P)
{
  if (++g_fail <= 20)
    std::printf("FAIL %s: mode %d C %d W %d H %d n %d pc %d piped %d form %d half %d chunk %d mx %d halfmode %d in.pitch %zu\n", what, in.mode, in.C, in.W, in.H, in.n,
                in.per_channel, (int)in.piped, P.form, P.fp.half, in.o.chunk, in.o.mx_mode, in.o.half_mode, in.in.pitch);
}
#define CHECK(cond, what) do { if (!(cond)) bad(what, in, P); } while (0)

// ---- the digest: FNV-1a over every field of every FrontPlan, in the order the driver makes them -------------------
static unsigned long long g_digest = 0xcbf29ce484222325ull;
static void fold_byte(unsigned b) { g_digest = (g_digest ^ (b & 0xFFu)) * 0x100000001b3ull; }
template <class T> static void fold(T v)  // an integer of any width, low byte first
{
  const unsigned long long u = (unsigned long long)v;
  for (unsigned k = 0; k < sizeof(T); ++k) fold_byte((unsigned)(u >> (8 * k)));
}
template <class T> static void fold(T *p) { fold((uintptr_t)p); }  // (every pointer of a plan is null: hipcanny.hip patches them in)
static void fold(bool b) { fold_byte(b ? 1 : 0); }
static void fold(const char *s) { for (; s && *s; ++s) fold_byte((unsigned char)*s); fold_byte(0); }
static void fold(const View &v) { fold(v.p); fold(v.pitch); fold(v.fs); }
static void fold(const FrontPlan &P)
{
  const FrontParams &f = P.fp;
  fold(P.error); fold(P.in_staged); fold(P.out_staged); fold(P.gray); fold(P.src); fold(P.mono); fold(P.dst);
  fold(P.form); fold(P.prov); fold(P.zeroed_words); fold(P.waves); fold(P.mask); fold(P.mask_a);
  fold(f.in); fold(f.bgr); fold(f.in_pitch); fold(f.in_frame_stride); fold(f.sbits); fold(f.cbits); fold(f.RD); fold(f.W); fold(f.H);
  fold(f.nstrips); fold(f.nchunks); fold(f.nframes);
#ifdef HC_LEGACY_FRONT
  // The legacy build's digest leaves out two values that no kernel reads, and nothing else: `subchunks` in plans of any
  // form but HC_FORM_FRONT4 (only k_front and launch_front use it) and `run_rows` in plans of the 4-px Mode O forms
  // (k_front_o and k_front_o_ext go by chunk_rows).  The commit the golden digest comes from filled both for every form
  // in one block that later code overwrote or left unread; the planner of today fills what the form's kernel reads.
  if (P.form == HC_FORM_FRONT4) fold(f.subchunks);
  if (!form_o_4px(P.form)) fold(f.run_rows);
#else
  fold(f.subchunks); fold(f.run_rows);
#endif
  fold(f.chunk_rows); fold(f.l2gradient); fold(f.total_items);
  for (int k = 0; k < 3; ++k) { fold(f.a_lo[k]); fold(f.a_hi[k]); }
  fold(f.blur); fold(f.blur_frame_stride); fold(f.nchunks_b); fold(f.run_rows_b); fold(f.total_items_b);
  fold(f.prov_out); fold(f.prov_pitch); fold(f.prov_fs); fold(f.dbg_blur); fold(f.dbg_pitch); fold(f.dbg_fs);
  fold(f.zeros); fold(f.dump); fold(f.dump_c); fold(f.dump_p); fold(f.zero_words); fold(f.zero_count);
  fold(f.half); fold(f.one_wave); fold(f.nhalf); fold(f.dense_enter); fold(f.dense_leave); fold(f.wrap_limit);
}
static FrontPlan plan_folded(const FrontIn &in)
{
  const FrontPlan P = plan_front(in);
  fold(P);
  return P;
}

struct Ctx {  // what hc_create / hc_set_option derive
  int mode, C, W, H, per_channel, max_batch, RD, nstrips;
  View own_in, own_mono, own_out;
  size_t dump_region, wl_cap;
};
static Ctx make_ctx(int mode, int C, int W, int H, int per_channel, int max_batch, bool force_half)
{
  Ctx c{ mode, C, W, H, per_channel, max_batch, plane_row_dwords(W), (W + STRIP_W - 1) / STRIP_W };
  c.own_in.pitch = frame_pitch(round_up((size_t)W, 8) * C, (size_t)W * C);
  c.own_out.pitch = frame_pitch((size_t)W, (size_t)W);
  c.own_mono.pitch = frame_pitch((size_t)W, 0);
  c.own_in.fs = c.own_in.pitch * H; c.own_out.fs = c.own_out.pitch * H; c.own_mono.fs = c.own_mono.pitch * H;
  c.own_in.p = c.own_mono.p = c.own_out.p = 0;
  c.dump_region = (half_pays(W) || force_half) ? half_dump_region(c.own_in.fs, c.own_out.fs, c.RD, H) : 0;
  c.wl_cap = slot_wl_cap((size_t)max_batch * (per_channel ? 3 : 1), H, c.RD);
  return c;
}
static FrontIn make_in(const Ctx &c, int n, bool piped, const FrontOpts &o, const View &in, const View &out, bool grads = false)
{
  FrontIn fi{ c.mode, c.C, c.W, c.H, c.RD, c.nstrips, c.per_channel, HC_STAGE_HYSTER, n };
  fi.in = in; fi.out = out; fi.in_dy = grads ? 0x30000000u : 0;
  fi.own_in = c.own_in; fi.own_mono = c.own_mono; fi.own_out = c.own_out;
  fi.o = o; fi.dump_region = c.dump_region; fi.piped = piped;
  fi.nslot_use = piped ? pipeline_slots(0, 2, c.per_channel ? 3 * n : n, c.W, c.H) : 2;
  fi.front_one = false; fi.out_overlap = false; fi.wl_cap = c.wl_cap;
  return fi;
}

// the claims of the issue, for one front plan and the hysteresis plans that can follow it
static void check(const Ctx &c, const FrontIn &in, const HystOpts &ho, bool full = true)
{
  const FrontPlan P = plan_folded(in);
  ++g_plans;
  if (P.error) {  // only the product build's refusal of the round-1 forms may appear in this sweep
    CHECK(in.mode == HC_MODE_R && in.o.split != 2, "unexpected plan error");
    return;
  }
  const FrontParams &f = P.fp;
  const int H = in.H, W = in.W, n_out = in.per_channel ? 3 * in.n : in.n;
  const long per = in.per_channel ? 3 : 1;
  const int rows = form_o_4px(P.form) ? f.chunk_rows : f.run_rows;
  CHECK(rows >= 1 && (long)f.nchunks * rows >= H, "nchunks * run_rows >= H");
  // the 4-px Mode O forms take hc_set_tuning's rows per work item as they are (any value >= 1, at most the frame)
  if (form_o_4px(P.form) && in.o.chunk)
    CHECK(f.chunk_rows == std::min(std::max(in.o.chunk, 1), H) && f.nchunks == (H + f.chunk_rows - 1) / f.chunk_rows, "4-px Mode O forms: chunk_rows = min(max(chunk, 1), H)");
  long units = (long)n_out * f.nstrips;
  if (P.form == HC_FORM_FRONT8_HALF) units = (((long)in.n * front8_half_strips(W) + 1) / 2) * per;
  if (P.form == HC_FORM_FRONT_MX) CHECK(f.nstrips == front_mx_strips(W), "mx strips");
  if (form_8px(P.form)) CHECK(f.nstrips == front8_strips(W) && (f.run_rows + 4) % F8_SUB == 0, "f8 strips / windows");
  CHECK(f.total_items > 0 && (long)f.total_items == units * f.nchunks, "total_items = units x chunks");
  if (form_8px(P.form))  // the dead `!can8` branch: rows always hold whole 8-pixel groups
    CHECK(f.in_pitch >= round_up((size_t)W, 8) * (size_t)(f.bgr ? 3 : 1), "8-px kernels read whole groups");
  CHECK((f.in_pitch | f.in_frame_stride) % (P.form == HC_FORM_O_GRADIENTS ? 2 : 4) == 0 && !reaches_4g(H, f.in_pitch), "input rows within 32-bit offsets, aligned");
  if (P.form == HC_FORM_FRONT8_HALF) {  // the `fits` inequalities, from the buffers the kernel really gets
    const size_t R = in.dump_region;
    CHECK(f.half == 1 && f.nhalf == front8_half_strips(W) && R != 0, "HALF parameters");
    CHECK(f.in_frame_stride + 32768 <= R && per * sizeof(u32) * (size_t)in.RD * H + 4096 <= R, "HALF: lane offsets fit the dump region");
    CHECK((unsigned long long)f.in_frame_stride + (unsigned long long)H * f.in_pitch < (1ull << 32), "HALF: input offsets below 4 GiB");
    if (P.prov) CHECK(per * f.prov_fs + 16384 <= R && (unsigned long long)per * f.prov_fs + (unsigned long long)H * f.prov_pitch < (1ull << 32), "HALF: provisional map offsets");
  } else CHECK(f.half == 0, "half only in HC_FORM_FRONT8_HALF");
  if (P.prov) CHECK(in.piped && (unsigned long long)H * P.dst.pitch < (1ull << 32) && f.prov_pitch == P.dst.pitch, "prov never with H * pitch >= 2^32");
  CHECK(P.zeroed_words <= run_flag_words(c.wl_cap) && f.zero_count == P.zeroed_words, "zeroed_words within d_flags");
  CHECK(P.waves == 0 || P.waves == 1 || P.waves == 3 || P.waves == 4, "waves per workgroup");
  // the hysteresis plans: fresh history, and histories that push every rule
  for (int hist = 0; hist < 4; hist += full ? 1 : 2) {
    HystHistory h;
    if (hist == 1) { h.need_rows = 64; h.last_work_launches = 3; }
    if (hist == 2) { h.need_rows = 40000; h.last_work_launches = 60; h.lists_last = true; h.obs[0] = 60; h.obs[1] = 50; }
    for (int rep = 0; rep < 2; ++rep) {
      const HystPlan p = plan_hyst(in.RD, H, n_out, in.piped, ho, h, c.wl_cap, P.zeroed_words);
      CHECK(p.fits && p.wl_stride <= c.wl_cap, "wl_stride <= wl_cap");
      CHECK(run_flag_words(p.wl_stride) <= run_flag_words(c.wl_cap), "flag words within d_flags");
      CHECK(p.K >= 1 && p.K <= MAX_HYST_LAUNCHES && WL_COUNT_WORDS >= p.K + 3, "1 <= K <= MAX_HYST_LAUNCHES");
      CHECK(p.nrtiles * p.tile_rows * p.waves >= H && p.wl_stride == (size_t)n_out * p.nrtiles * p.npanels, "tiles cover the frame");
      if (p.loop) CHECK(p.wl_stride <= (size_t)HYST_LOOP_MAX_TILES && !in.piped && p.npanels == 1 && hyst_shape_loops(p.tile_rows, p.waves), "loop form: small, whitelisted shape");
      for (int k = 0; k < p.K; ++k) {
        const int want = p.mixed ? (k < 2 ? 0 : k == 2 ? 2 : 1) : p.lists0;
        CHECK(p.lists[k] == want && (!p.loop || p.lists[k] == 0), "list modes 0..0, 2, 1..1");
        CHECK(p.late_grid[k] >= 0 && (size_t)p.late_grid[k] <= std::max<size_t>(p.wl_stride, (size_t)p.test_grid), "late grid");
      }
      if (p.mixed) CHECK(in.piped && !p.lists0 && !p.loop, "mixed only beside a front kernel");
      // the run finishes: the last launches found work (hist 3: every launch did, as a continued run reports)
      std::vector<u32> counts(MAX_HYST_LAUNCHES + 1, (u32)std::min<size_t>(p.wl_stride, 0xFFFFFFFFu));
      h.finished(p, hist == 3 ? 3 * p.K : std::min(p.K, 2 + hist), counts.data());
    }
  }
}

static void sweep_geometry(int W, int H, bool full)
{
  const HystOpts ho0;
  std::vector<int> batches = { 1, 8 };
  if (full) { batches.push_back(2); batches.push_back(64); }
  const long cross = (500l * 1000 * 1000 + (long)W * H - 1) / ((long)W * H);  // the first batch the slot rule calls big
  if (cross <= (1 << 20)) { batches.push_back((int)cross); if (cross > 1 && full) batches.push_back((int)cross - 1); }
  for (int mode : { HC_MODE_R, HC_MODE_O })
    for (int C : { 1, 3 })
      for (int pc = 0; pc <= (mode == HC_MODE_R && C == 3 ? 1 : 0); ++pc)
        for (int n : batches) {
          const int max_batch = n;
          for (int piped = 0; piped <= 1; ++piped) {
            std::vector<FrontOpts> opts(1);
            if (!full) {  // every geometry: the forms that cut the work their own way
              FrontOpts o;
              o.mx_mode = 1; opts.push_back(o);
              o = FrontOpts{}; o.half_mode = 1; opts.push_back(o);
              o = FrontOpts{}; o.chunk = 8; o.aperture = 5; opts.push_back(o);
            } else {
              FrontOpts o;
              for (int v : { 0, 1 }) { o = FrontOpts{}; o.half_mode = v; opts.push_back(o); }
              o = FrontOpts{}; o.mx_mode = 1; opts.push_back(o);
              o.half_mode = 0; opts.push_back(o);
              for (int v : { 0, 1 }) { o = FrontOpts{}; o.dense_mode = v; opts.push_back(o); }
              for (int v : { 1, 4 }) { o = FrontOpts{}; o.wpb_mode = v; o.mx_mode = v == 1; opts.push_back(o); }
              for (int v : { 8, 50, 300, 16384 }) { o = FrontOpts{}; o.chunk = v; o.half_mode = v == 50; o.mx_mode = v == 300; opts.push_back(o); }
              o = FrontOpts{}; o.nms_saturate = 1; o.debug_taps = true; opts.push_back(o);
              o = FrontOpts{}; o.split = 1; opts.push_back(o);
              o.split = 0; opts.push_back(o);
              if (mode == HC_MODE_O) { o = FrontOpts{}; o.aperture = 5; opts.push_back(o); o.l2gradient = 1; opts.push_back(o); o.aperture = 3; opts.push_back(o); }
              if (mode == HC_MODE_O)  // work items of 1, 7 and 17 rows: k_front_o (split 0 / 3 channels), k_front_o_ext (aperture 5; gradients below)
                for (int v : { 1, 7, 17 }) { o = FrontOpts{}; o.chunk = v; o.split = 0; opts.push_back(o); o.aperture = 5; opts.push_back(o); }
            }
            for (const FrontOpts &o : opts) {
              const Ctx c = make_ctx(mode, C, W, H, pc, max_batch, o.half_mode == 1);
              const size_t tight = (size_t)W * C;
              const View out{ 0x20000000u, (size_t)W, (size_t)W * H };
              std::vector<View> ins = { View{ 0x10000000u, tight, tight * H }, View{ 0x10000000u, c.own_in.pitch, c.own_in.fs } };
              if (full) { ins.push_back(View{ 0x10000001u, tight + 3, (tight + 3) * H }); ins.push_back(View{ 0x10000000u, round_up(tight, 4) + 4096, (round_up(tight, 4) + 4096) * H }); }
              if (!full) { check(c, make_in(c, n, piped != 0, o, ins[(W + H + n) & 1], out), ho0, false); continue; }
              for (const View &v : ins) check(c, make_in(c, n, piped != 0, o, v, out), ho0);
              if (full) {
                check(c, make_in(c, n, piped != 0, o, ins[0], View{ 0x20000002u, (size_t)W + 1, ((size_t)W + 1) * H }), ho0);  // staged output
                HystOpts ho;
                for (int g : { -1, 1, 7 }) { ho = HystOpts{}; ho.late_grid = g; check(c, make_in(c, n, piped != 0, o, ins[0], out), ho); }
                ho = HystOpts{}; ho.loop = false; ho.diag = true; check(c, make_in(c, n, piped != 0, o, ins[0], out), ho);
                for (const HystShape &g : HYST_SHAPES) { ho = HystOpts{}; ho.geom = g.tile_rows * 100 + g.waves; check(c, make_in(c, n, piped != 0, o, ins[0], out), ho); }
                for (int k : { 1, 6, 96 }) { ho = HystOpts{}; ho.launches = k; ho.launches_set = true; check(c, make_in(c, n, piped != 0, o, ins[0], out), ho); }
                if (mode == HC_MODE_O) check(c, make_in(c, n, piped != 0, o, View{ 0x10000000u, 2 * tight + 2, (2 * tight + 2) * H }, out, true), ho0);
              }
            }
          }
        }
}

// forms the GPU tests pin (tests/test_gpu_half_strips.py, test_gpu_front_mx.py, test_gpu_canny_o_ext.py, test_gpu_views.py,
// __graft_entry__.py): (input staged, output staged, form)
static void expect(const char *what, const Ctx &c, int n, bool piped, const FrontOpts &o, const View &in, const View &out, int staged_in, int staged_out, int form, bool grads = false)
{
  const FrontPlan P = plan_folded(make_in(c, n, piped, o, in, out, grads));
  if (P.error || P.form != form || (staged_in >= 0 && P.in_staged != (staged_in != 0)) || (staged_out >= 0 && P.out_staged != (staged_out != 0))) {
    ++g_fail;
    std::printf("FAIL pinned %s: got (%d, %d, %d)%s\n", what, (int)P.in_staged, (int)P.out_staged, P.form, P.error ? P.error : "");
  }
}
// the work split of the 4-px Mode O forms: (form, rows per work item, items per strip, items)
static void expect_cut(const char *what, const Ctx &c, int n, const FrontOpts &o, bool grads, int form, int chunk_rows, int nchunks, int total_items)
{
  const View in = grads ? View{ 0x10000000u, (size_t)2 * c.C * c.W, (size_t)2 * c.C * c.W * c.H } : c.own_in;
  const FrontPlan P = plan_folded(make_in(c, n, false, o, in, c.own_out, grads));
  if (P.error || P.form != form || P.fp.chunk_rows != chunk_rows || P.fp.nchunks != nchunks || P.fp.total_items != total_items) {
    ++g_fail;
    std::printf("FAIL pinned cut %s: got form %d, %d rows x %d, %d items%s\n", what, P.form, P.fp.chunk_rows, P.fp.nchunks, P.fp.total_items, P.error ? P.error : "");
  }
}
// the work split of the 8-px forms on the contexts' internal buffers (hc_run): (form, rows per run, runs per strip, items)
static void expect_runs(const char *what, const Ctx &c, int n, const FrontOpts &o, int form, int run_rows, int nchunks, int total_items)
{
  const FrontPlan P = plan_folded(make_in(c, n, false, o, c.own_in, c.own_out));
  if (P.error || P.form != form || P.in_staged || P.out_staged || P.fp.run_rows != run_rows || P.fp.nchunks != nchunks || P.fp.total_items != total_items) {
    ++g_fail;
    std::printf("FAIL pinned runs %s (%d x %d, set length %d): got form %d, %d rows x %d, %d items%s\n", what, c.W, c.H, o.chunk, P.form, P.fp.run_rows, P.fp.nchunks, P.fp.total_items, P.error ? P.error : "");
  }
}
// ... and of its pipelined leg: tight device buffers (hc_run_device), nothing staged, and the front kernel writes the provisional map
static void expect_prov(const char *what, const Ctx &c, int n, const FrontOpts &o, int form, int run_rows, int nchunks, int total_items)
{
  const View in{ 0x10000000u, (size_t)c.W * c.C, (size_t)c.W * c.C * c.H }, out{ 0x20000000u, (size_t)c.W, (size_t)c.W * c.H };
  const FrontPlan P = plan_folded(make_in(c, n, true, o, in, out));
  if (P.error || P.form != form || P.in_staged || P.out_staged || !P.prov || P.fp.prov_pitch != (u32)c.W || P.fp.prov_fs != (size_t)c.W * c.H
      || P.fp.run_rows != run_rows || P.fp.nchunks != nchunks || P.fp.total_items != total_items) {
    ++g_fail;
    std::printf("FAIL pinned pipelined %s (%d x %d, set length %d): got form %d, prov %d, staged %d %d, %d rows x %d, %d items%s\n", what, c.W, c.H, o.chunk, P.form, (int)P.prov,
                (int)P.in_staged, (int)P.out_staged, P.fp.run_rows, P.fp.nchunks, P.fp.total_items, P.error ? P.error : "");
  }
}
// tests/test_gpu_front8_runs.py (tests/front8_runs_inputs.py): batches of three frames, hc_set_tuning's length -> the runs
static void pinned_front8_runs()
{
  FrontOpts f8; f8.half_mode = 0;
  FrontOpts half; half.half_mode = 1;
  FrontOpts mx; mx.half_mode = 0; mx.mx_mode = 1;
  const FrontOpts fo;  // Mode O: k_front8o by default
  FrontOpts l2o; l2o.l2gradient = 1;
  auto with = [](FrontOpts o, int chunk, int dense = -1) { o.chunk = chunk; o.dense_mode = dense; return o; };
  {  // leg B: 41 rows, every distinct run length 6 k - 4, the frame, beyond it; 504 columns: two strips, six units
    const Ctx c = make_ctx(HC_MODE_R, 1, 504, 41, 0, 3, false), co = make_ctx(HC_MODE_O, 1, 504, 41, 0, 3, false);
    const int cut[][3] = { { 2, 2, 21 }, { 8, 8, 6 }, { 14, 14, 3 }, { 20, 20, 3 }, { 26, 26, 2 }, { 32, 32, 2 }, { 38, 38, 2 }, { 41, 44, 1 }, { 100, 44, 1 } };
    for (const auto &k : cut) {
      expect_runs("k_front8 mono", c, 3, with(f8, k[0]), HC_FORM_FRONT8, k[1], k[2], 6 * k[2]);
      expect_runs("k_front8o", co, 3, with(fo, k[0]), HC_FORM_FRONT8O, k[1], k[2], 6 * k[2]);
    }
    FrontOpts l2 = with(fo, 26); l2.l2gradient = 1;
    expect_runs("k_front8o L2, a second strip of one column", make_ctx(HC_MODE_O, 1, 497, 41, 0, 3, false), 3, l2, HC_FORM_FRONT8O, 26, 2, 12);
    expect_runs("k_front8, one strip", make_ctx(HC_MODE_R, 1, 496, 41, 0, 3, false), 3, with(f8, 14), HC_FORM_FRONT8, 14, 3, 9);
  }
  {  // leg A: the last run of every length comes from heights 1 .. 22 under runs of 2, 8 and 14 rows
    const int cut[][4] = { { 1, 2, 2, 1 }, { 1, 8, 2, 1 }, { 3, 2, 2, 2 }, { 3, 14, 8, 1 }, { 4, 8, 8, 1 }, { 5, 8, 8, 1 }, { 7, 2, 2, 4 }, { 8, 14, 8, 1 },
                           { 9, 8, 8, 2 }, { 9, 14, 14, 1 }, { 15, 14, 14, 2 }, { 16, 8, 8, 2 }, { 17, 8, 8, 3 }, { 21, 2, 2, 11 }, { 21, 14, 14, 2 }, { 22, 14, 14, 2 }, { 22, 2, 2, 11 },
                           { 8, 0, 8, 1 }, { 21, 0, 14, 2 }, { 22, 0, 14, 2 } };  // (0: the automatic split of a small batch)
    for (const auto &k : cut) {
      expect_runs("k_front8 heights", make_ctx(HC_MODE_R, 1, 504, k[0], 0, 3, false), 3, with(f8, k[1]), HC_FORM_FRONT8, k[2], k[3], 6 * k[3]);
      expect_runs("k_front8o heights", make_ctx(HC_MODE_O, 1, 504, k[0], 0, 3, false), 3, with(fo, k[1]), HC_FORM_FRONT8O, k[2], k[3], 6 * k[3]);
    }
    expect_runs("tiny", make_ctx(HC_MODE_R, 1, 5, 7, 0, 3, false), 3, with(f8, 2), HC_FORM_FRONT8, 2, 4, 12);
    expect_runs("tiny, half", make_ctx(HC_MODE_R, 1, 5, 7, 0, 3, true), 3, with(half, 2), HC_FORM_FRONT8_HALF, 2, 4, 8);
  }
  // each form once: dense forced, BGR -> grey, per-channel (nine output frames)
  expect_runs("k_front8 dense", make_ctx(HC_MODE_R, 1, 504, 21, 0, 3, false), 3, with(f8, 8, 1), HC_FORM_FRONT8, 8, 3, 18);
  expect_runs("k_front8 BGR", make_ctx(HC_MODE_R, 3, 504, 21, 0, 3, false), 3, with(f8, 14), HC_FORM_FRONT8, 14, 2, 12);
  expect_runs("k_front8 per-channel", make_ctx(HC_MODE_R, 3, 504, 21, 1, 3, false), 3, with(f8, 2), HC_FORM_FRONT8, 2, 11, 198);
  // the half-strip form: 488 columns are three half-strips, nine units, five pairs; 241 columns two, three pairs; 240 one, two pairs
  expect_runs("half mono", make_ctx(HC_MODE_R, 1, 488, 41, 0, 3, true), 3, with(half, 8), HC_FORM_FRONT8_HALF, 8, 6, 30);
  expect_runs("half mono dense", make_ctx(HC_MODE_R, 1, 488, 21, 0, 3, true), 3, with(half, 14, 1), HC_FORM_FRONT8_HALF, 14, 2, 10);
  expect_runs("half BGR", make_ctx(HC_MODE_R, 3, 241, 41, 0, 3, true), 3, with(half, 20), HC_FORM_FRONT8_HALF, 20, 3, 9);
  expect_runs("half per-channel", make_ctx(HC_MODE_R, 3, 488, 41, 1, 3, true), 3, with(half, 2), HC_FORM_FRONT8_HALF, 2, 21, 315);
  expect_runs("half, one half-strip", make_ctx(HC_MODE_R, 1, 240, 41, 0, 3, true), 3, with(half, 38), HC_FORM_FRONT8_HALF, 38, 2, 4);
  {  // k_front_mx: ceil(H / c) runs of ceil(H / runs) rows; 224 columns: two strips, six units.  Both sides of the block
     // borders front_mx_run_rows(1) = 12 and (2) = 28, a last run of 1 and of 16 rows, runs of one row, the frame
    if (front_mx_run_rows(1) != 12 || front_mx_run_rows(2) != 28) { ++g_fail; std::printf("FAIL front_mx_run_rows\n"); }
    const int cut[][4] = { { 24, 12, 12, 2 }, { 25, 13, 13, 2 }, { 26, 13, 13, 2 }, { 36, 12, 12, 3 }, { 39, 13, 13, 3 }, { 56, 28, 28, 2 }, { 57, 29, 29, 2 }, { 58, 29, 29, 2 },
                           { 84, 28, 28, 3 }, { 87, 29, 29, 3 }, { 3, 2, 2, 2 }, { 33, 17, 17, 2 }, { 21, 8, 7, 3 }, { 21, 14, 11, 2 }, { 41, 1, 1, 41 }, { 41, 6, 6, 7 }, { 41, 14, 14, 3 },
                           { 41, 21, 21, 2 }, { 41, 41, 41, 1 }, { 41, 100, 41, 1 } };
    for (const auto &k : cut) expect_runs("k_front_mx", make_ctx(HC_MODE_R, 1, 224, k[0], 0, 3, false), 3, with(mx, k[1]), HC_FORM_FRONT_MX, k[2], k[3], 6 * k[3]);
    expect_runs("k_front_mx, a second strip of one column", make_ctx(HC_MODE_R, 1, 217, 41, 0, 3, false), 3, with(mx, 9), HC_FORM_FRONT_MX, 9, 5, 30);
    expect_runs("k_front_mx, one strip", make_ctx(HC_MODE_R, 1, 216, 41, 0, 3, false), 3, with(mx, 11), HC_FORM_FRONT_MX, 11, 4, 12);
  }
  // the pipelined leg: 41 rows at the provisional-map width of each kernel; every form keeps its provisional map (the
  // half-strip form: the `fits` terms with the map, per-channel with three maps per frame)
  expect_prov("k_front8 mono", make_ctx(HC_MODE_R, 1, 504, 41, 0, 3, false), 3, with(f8, 8), HC_FORM_FRONT8, 8, 6, 36);
  expect_prov("k_front8 dense", make_ctx(HC_MODE_R, 1, 504, 41, 0, 3, false), 3, with(f8, 2, 1), HC_FORM_FRONT8, 2, 21, 126);
  expect_prov("k_front8 BGR", make_ctx(HC_MODE_R, 3, 504, 41, 0, 3, false), 3, with(f8, 14), HC_FORM_FRONT8, 14, 3, 18);
  expect_prov("k_front8 per-channel", make_ctx(HC_MODE_R, 3, 504, 41, 1, 3, false), 3, with(f8, 100), HC_FORM_FRONT8, 44, 1, 18);
  expect_prov("half mono", make_ctx(HC_MODE_R, 1, 488, 41, 0, 3, true), 3, with(half, 2), HC_FORM_FRONT8_HALF, 2, 21, 105);
  expect_prov("half mono dense", make_ctx(HC_MODE_R, 1, 488, 41, 0, 3, true), 3, with(half, 20, 1), HC_FORM_FRONT8_HALF, 20, 3, 15);
  expect_prov("half BGR", make_ctx(HC_MODE_R, 3, 488, 41, 0, 3, true), 3, with(half, 41), HC_FORM_FRONT8_HALF, 44, 1, 5);
  expect_prov("half per-channel", make_ctx(HC_MODE_R, 3, 488, 41, 1, 3, true), 3, with(half, 8), HC_FORM_FRONT8_HALF, 8, 6, 90);
  expect_prov("k_front8o", make_ctx(HC_MODE_O, 1, 504, 41, 0, 3, false), 3, with(fo, 26), HC_FORM_FRONT8O, 26, 2, 12);
  expect_prov("k_front8o L2", make_ctx(HC_MODE_O, 1, 504, 41, 0, 3, false), 3, with(l2o, 38), HC_FORM_FRONT8O, 38, 2, 12);
  expect_prov("k_front_mx", make_ctx(HC_MODE_R, 1, 224, 41, 0, 3, false), 3, with(mx, 6), HC_FORM_FRONT_MX, 6, 7, 42);
  expect_prov("k_front_mx, runs of one row", make_ctx(HC_MODE_R, 1, 224, 41, 0, 3, false), 3, with(mx, 1), HC_FORM_FRONT_MX, 1, 41, 246);
}

static void pinned()
{
  FrontOpts d, o;
  auto tight = [](const Ctx &c) { return View{ 0x10000000u, (size_t)c.W * c.C, (size_t)c.W * c.C * c.H }; };
  auto tout = [](const Ctx &c) { return View{ 0x20000000u, (size_t)c.W, (size_t)c.W * c.H }; };
  {  // test_half_form_pipelined_device_buffers: 640 x 480, 5 frames, pipelined
    const Ctx c = make_ctx(HC_MODE_R, 1, 640, 480, 0, 5, false);
    o = d; expect("half auto", c, 5, true, o, tight(c), tout(c), 0, 0, HC_FORM_FRONT8_HALF);
    o.half_mode = 0; expect("half 0", c, 5, true, o, tight(c), tout(c), 0, 0, HC_FORM_FRONT8);
    o.half_mode = 1; expect("half 1", c, 5, true, o, tight(c), tout(c), 0, 0, HC_FORM_FRONT8_HALF);
  }
  for (int chunk : { 8, 20, 50, 300 }) {  // test_half_form_run_lengths_and_thresholds (hc_run: the internal buffers)
    const Ctx c = make_ctx(HC_MODE_R, 1, 640, 230, 0, 3, true);
    o = d; o.half_mode = 1; o.chunk = chunk; expect("half chunk", c, 3, false, o, c.own_in, c.own_out, -1, -1, HC_FORM_FRONT8_HALF);
  }
  for (int w : { 96, 500, 640, 1000 })  // test_half_form_three_channel
    for (int pc : { 0, 1 }) {
      const Ctx c = make_ctx(HC_MODE_R, 3, w, 70, pc, 3, true);
      o = d; o.half_mode = 1; o.debug_taps = true; expect("half 3ch", c, 3, false, o, c.own_in, c.own_out, -1, -1, HC_FORM_FRONT8_HALF);
    }
  {  // __graft_entry__.py smoke: 640 x 480 x 2 with HC_OPT_FRONT_MX
    const Ctx c = make_ctx(HC_MODE_R, 1, 640, 480, 0, 2, false);
    o = d; o.mx_mode = 1; expect("smoke mx", c, 2, false, o, c.own_in, c.own_out, -1, -1, HC_FORM_FRONT_MX);
  }
  for (int ap5 = 0; ap5 <= 1; ++ap5)  // test_gpu_canny_o_ext: aperture 5 -> 6, gradients -> 7
    for (int C : { 1, 3 }) {
      const Ctx c = make_ctx(HC_MODE_O, C, 322, 97, 0, 2, false);
      o = d; o.aperture = ap5 ? 5 : 3;
      if (ap5) expect("aperture 5", c, 2, false, o, c.own_in, c.own_out, -1, -1, HC_FORM_O_APERTURE5);
      expect("gradients", c, 2, true, o, View{ 0x10000000u, (size_t)2 * C * 322 + 4, ((size_t)2 * C * 322 + 4) * 97 }, tout(c), 0, -1, HC_FORM_O_GRADIENTS, true);
    }
  {  // the automatic work split of the 4-px Mode O forms (hc_set_tuning 0): ceil(12288 / (frames x strips)) items per strip, of 16 rows or more
    FrontOpts a5 = d; a5.aperture = 5;
    const Ctx one = make_ctx(HC_MODE_O, 3, 322, 97, 0, 1, false);  // one frame, two strips: 7 items of 14 rows per strip
    expect_cut("one frame", one, 1, d, false, HC_FORM_FRONT_O, 14, 7, 14);
    expect_cut("one frame, aperture 5", one, 1, a5, false, HC_FORM_O_APERTURE5, 14, 7, 14);
    expect_cut("one frame, gradients", one, 1, d, true, HC_FORM_O_GRADIENTS, 14, 7, 14);
    const Ctx hd = make_ctx(HC_MODE_O, 1, 1920, 1080, 0, 1024, false);  // 1024 frames of 1080p: 8192 strips, two items of 540 rows each
    expect_cut("1080p x 1024, aperture 5", hd, 1024, a5, false, HC_FORM_O_APERTURE5, 540, 2, 16384);
    // test_gpu_mode_o_chunks.py: one strip, 6144 frames -> two items per strip, 12288 -> one spans the frame
    const Ctx s3 = make_ctx(HC_MODE_O, 3, 64, 26, 0, 12288, false), s1 = make_ctx(HC_MODE_O, 1, 64, 26, 0, 12288, false);
    expect_cut("two per strip", s3, 6144, d, false, HC_FORM_FRONT_O, 13, 2, 12288);
    expect_cut("one per strip", s3, 12288, d, false, HC_FORM_FRONT_O, 26, 1, 12288);
    expect_cut("two per strip, aperture 5", s1, 6144, a5, false, HC_FORM_O_APERTURE5, 13, 2, 12288);
    expect_cut("one per strip, aperture 5", s1, 12288, a5, false, HC_FORM_O_APERTURE5, 26, 1, 12288);
    expect_cut("two per strip, gradients", s1, 6144, d, true, HC_FORM_O_GRADIENTS, 13, 2, 12288);
    expect_cut("one per strip, gradients", s1, 12288, d, true, HC_FORM_O_GRADIENTS, 26, 1, 12288);
    for (int chunk : { 1, 7, 17, 300 }) {  // ... and a set length, as it is
      FrontOpts t = a5; t.chunk = chunk;
      const int rows = std::min(chunk, 97), items = (97 + rows - 1) / rows;
      expect_cut("set length", one, 1, t, false, HC_FORM_O_APERTURE5, rows, items, 2 * items);
    }
  }
  for (int mx = 0; mx <= 1; ++mx) {  // test_gpu_views: a 4 GiB-reaching view of a wide parent, w x h = 64 x 1024 rows of a 4 MiB pitch
    const int w = 64, h = 1024;
    const size_t pitch = (size_t)4 << 20;
    const Ctx c = make_ctx(HC_MODE_R, 1, w, h, 0, 1, false);
    o = d; o.half_mode = 0; o.mx_mode = mx;
    const View far{ 0x40000000u, pitch, pitch * h };
    FrontIn fi = make_in(c, 1, true, o, tight(c), far);
    const FrontPlan P = plan_folded(fi);
    if (P.prov || P.in_staged || P.out_staged || P.form != (mx ? HC_FORM_FRONT_MX : HC_FORM_FRONT8)) { ++g_fail; std::printf("FAIL pinned far output view\n"); }
    expect("far input view", c, 1, true, o, far, tout(c), 1, 0, mx ? HC_FORM_FRONT_MX : HC_FORM_FRONT8);
  }
  {  // non-final stages plan no front kernel
    const Ctx c = make_ctx(HC_MODE_R, 3, 100, 50, 0, 2, false);
    FrontIn fi = make_in(c, 2, false, d, tight(c), tout(c));
    fi.stage = HC_STAGE_NMS;
    const FrontPlan P = plan_folded(fi);
    if (P.form != HC_FORM_FRONT_O || P.in_staged || P.out_staged || !P.gray) { ++g_fail; std::printf("FAIL pinned stage tap\n"); }
  }
}

// ChainWatch against the rules stated above it
#define WCHECK(cond, what) do { if (!(cond)) { ++g_fail; std::printf("FAIL ChainWatch: %s (line %d)\n", what, __LINE__); } } while (0)
static void chain_watch()
{
  auto step = [](ChainWatch &w, unsigned long long &i, float front, float lead) { ++i; w.update(i, pipeline_slots(w.pipe_slots, w.big_slots, 1 << 20, 1920, 1080), front, lead); };
  {  // three outlasting runs, but never before run 5
    ChainWatch w; unsigned long long i = 1;
    step(w, i, 1.0f, -0.1f); step(w, i, 1.0f, -0.1f); step(w, i, 1.0f, -0.1f);  // runs 2, 3, 4
    WCHECK(w.big_slots == 2 && w.chain_bound_runs == 3, "no trial before run 5");
    step(w, i, 1.0f, -0.1f);  // run 5
    WCHECK(w.big_slots == 3 && w.trial_runs == 0, "trial at run 5 after three outlasting runs");
    // the trial: ten runs; 0.98 of the old step is not enough -> back, wait 64, back-off doubles
    for (int k = 0; k < 9; ++k) { step(w, i, 0.98f, -0.1f); WCHECK(w.big_slots == 3, "trial lasts ten runs"); }
    step(w, i, 0.98f, -0.1f);
    WCHECK(w.big_slots == 2 && w.retry_wait == 64 && w.retry_backoff == 128, "trial that did not pay: back-off 64, doubling");
    int waited = 0;
    while (w.big_slots == 2 && waited < 200) { step(w, i, 1.0f, -0.1f); ++waited; }
    WCHECK(waited == 64, "next trial after 64 runs");
    for (int k = 0; k < 10; ++k) step(w, i, 0.96f, -0.1f);
    WCHECK(w.big_slots == 3 && w.trial_runs == -1, "kept below 0.97 x the pre-trial mean");
    // 16 light runs -> two slots, the next time 32
    for (int k = 0; k < 15; ++k) step(w, i, 0.96f, 0.01f);
    WCHECK(w.big_slots == 3, "15 light runs keep the slot");
    step(w, i, 0.96f, 0.01f);
    WCHECK(w.big_slots == 2 && w.chain_light_needed == 32, "two slots after 16 light runs, doubling");
  }
  {  // the caps: 4096 and 1024
    ChainWatch w; unsigned long long i = 10;
    for (int t = 0; t < 12; ++t) {
      while (w.big_slots == 2) step(w, i, 1.0f, -0.1f);
      for (int k = 0; k < 10; ++k) step(w, i, 1.0f, -0.1f);
    }
    WCHECK(w.retry_backoff == 4096, "back-off doubles to 4096");
    ChainWatch v; i = 10;
    for (int t = 0; t < 10; ++t) {
      v.retry_wait = 0;
      while (v.big_slots == 2) step(v, i, 1.0f, -0.1f);
      for (int k = 0; k < 10; ++k) step(v, i, 0.5f, -0.1f);  // kept
      WCHECK(v.big_slots == 3, "kept");
      while (v.big_slots == 3) step(v, i, 0.5f, 0.01f);
      for (int k = 0; k < 4; ++k) step(v, i, 1.0f, 0.01f);  // the old step again
    }
    WCHECK(v.chain_light_needed == 1024, "light runs needed double to 1024");
  }
  {  // one wave above 0.25, four below 0.03
    ChainWatch w; unsigned long long i = 1;
    step(w, i, 1.0f, 0.9f);
    WCHECK(!w.front_one, "ema 0.225");
    step(w, i, 1.0f, 0.9f);
    WCHECK(w.front_one && w.slack_ema > 0.25f, "one wave above 0.25");
    while (w.slack_ema >= 0.03f) { WCHECK(w.front_one, "stays until below 0.03"); step(w, i, 1.0f, 0.0f); }
    WCHECK(!w.front_one, "four waves below 0.03");
    step(w, i, 0.0f, 0.5f);
    WCHECK(w.slack_ema < 0.03f, "a run without a front time changes nothing");
  }
  {  // chain_told: +1 every chain outlasts and the trial is kept; -1 nothing outlasts; fixed slots: no trials
    ChainWatch w; w.chain_told = 1; unsigned long long i = 1;
    for (int k = 0; k < 4; ++k) step(w, i, 1.0f, 0.5f);
    WCHECK(w.big_slots == 3, "told +1: trial although the chains end early");
    for (int k = 0; k < 10; ++k) step(w, i, 2.0f, 0.5f);
    WCHECK(w.big_slots == 3, "told +1: kept although slower");
    for (int k = 0; k < 100; ++k) step(w, i, 2.0f, 0.5f);
    WCHECK(w.big_slots == 3, "told +1: no light runs");
    ChainWatch v; v.chain_told = -1; i = 1;
    for (int k = 0; k < 50; ++k) step(v, i, 1.0f, -0.5f);
    WCHECK(v.big_slots == 2, "told -1: no trial although the chains outlast");
    ChainWatch f; f.pipe_slots = 2; i = 1;
    for (int k = 0; k < 50; ++k) step(f, i, 1.0f, -0.5f);
    WCHECK(f.big_slots == 2 && pipeline_slots(f.pipe_slots, f.big_slots, 1, 8, 8) == 2 && pipeline_depth(true, 2, 2, 1, 8, 8) == 2, "fixed slots");
    WCHECK(pipeline_slots(0, 2, 241, 1920, 1080) == 4 && pipeline_slots(0, 2, 242, 1920, 1080) == 2 && pipeline_depth(true, 0, 2, 242, 1920, 1080) == 3 && pipeline_depth(false, 0, 2, 1, 8, 8) == 1, "0.5 G-pixel slot rule");
  }
}

// ---- check_view and the plans of the entries that are not runs ----------------------------------------------------
// (no front plans: they are neither counted in g_plans nor folded into the digest)
#define VCHECK(cond, ...) do { if (!(cond) && ++g_fail <= 20) { std::printf("FAIL line %d: ", __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)
struct ViewSpec { const char *entry; size_t row_bytes; unsigned align; bool below_4g; };

// Each entry's view specification (hipcanny.hip, device_ops.hip) on frames of W x H x C: the tight view and a padded, offset one pass; each
// single defect is reported as its own rule -- the cases of test_gpu_derivatives.py::test_errors and of the `bad` table of
// test_gpu_edge_points.py -- and no pitch gets past through a height * pitch that wrapped 64 bits.
static void view_table(int W, int H, int C)
{
  const size_t u8 = (size_t)W * C, i16 = 2 * u8, G4 = (size_t)1 << 32, top = SIZE_MAX;
  const ViewSpec specs[] = { { "hc_run_device / hc_canny_device in", u8, 1, false }, { "run / canny / gradients / hysteresis out, hysteresis in", (size_t)W, 1, false },
                             { "hc_run_gradients_device dx / dy", i16, 2, false }, { "hc_derivatives_device in, histogram entries", u8, 1, true },
                             { "hc_derivatives_device dx / dy", i16, 2, true }, { "hc_edge_points_device map", (size_t)W, 1, true } };
  const uintptr_t base = 0x10000000u;
  for (const ViewSpec &s : specs) {
    const size_t row = s.row_bytes, a = s.align, fs = row * H;
    auto rule = [&](uintptr_t p, size_t pitch, size_t stride, int n) { return check_view(View{ p, pitch, stride }, row, H, n, s.align, s.below_4g); };
    VCHECK(rule(base, row, fs, 2) == VIEW_OK && rule(base, row, fs, 1) == VIEW_OK, "%s: tight view", s.entry);
    VCHECK(rule(base + a, row + 3 * a, (row + 3 * a) * H + 5 * a, 2) == VIEW_OK, "%s: padded view at an offset", s.entry);
    VCHECK(rule(base, row - 1, fs, 1) == VIEW_PITCH && rule(base, 0, fs, 2) == VIEW_PITCH, "%s: pitch = row - 1", s.entry);
    VCHECK(rule(base, row, fs - 1, 2) == VIEW_STRIDE && rule(base, row + a, fs, 2) == VIEW_STRIDE, "%s: stride = pitch * H - 1, n = 2", s.entry);
    VCHECK(rule(base, row, fs - a, 1) == VIEW_OK && rule(base, row, 0, 1) == VIEW_OK, "%s: one frame has no stride to keep", s.entry);
    if (a == 1) VCHECK(rule(base + 1, row + 1, (row + 1) * H + 1, 2) == VIEW_OK && rule(base, row, fs - 1, 1) == VIEW_OK, "%s: u8 views of any alignment", s.entry);
    if (a == 2) {
      VCHECK(rule(base + 1, row, fs, 2) == VIEW_ALIGN && rule(base, row + 1, (row + 1) * H + (H & 1), 2) == VIEW_ALIGN && rule(base, row, fs + 1, 2) == VIEW_ALIGN
             && rule(base, row, fs + 1, 1) == VIEW_ALIGN, "%s: odd address, pitch, stride", s.entry);
      VCHECK(rule(base + 2, row + 2, (row + 2) * H + 2, 2) == VIEW_OK, "%s: even is enough", s.entry);
    }
    // both sides of 4 GiB: height * pitch = 2^32 exactly (where H divides it), the last pitch of this alignment below, the first at or above
    const ViewFault far = s.below_4g ? VIEW_4G : VIEW_OK;
    const size_t first = (G4 + H - 1) / H, at = (first + 3) / 4 * 4, under = (G4 - 1) / H / 4 * 4;
    VCHECK((unsigned long long)H * at >= G4 && (unsigned long long)H * under < G4 && (G4 % H || H * first == G4), "the limit itself");
    VCHECK(rule(base, at, at * H, 2) == far && rule(base, at, fs, 1) == far, "%s: H * pitch reaches 2^32", s.entry);
    if (under >= row) VCHECK(rule(base, under, under * H, 2) == VIEW_OK && rule(base, under, fs, 1) == VIEW_OK, "%s: H * pitch just below 2^32", s.entry);
    VCHECK(rule(base, (size_t)1 << 31, ((size_t)1 << 31) * H, 2) == (H > 1 ? far : VIEW_OK) && rule(base, G4 / H, G4 / H * H, 1) == (a == 2 && (G4 / H & 1) ? VIEW_ALIGN : G4 % H ? VIEW_OK : far), "%s: pitch 1 << 31, (1 << 32) / H", s.entry);
    VCHECK(reaches_4g(H, at) && !reaches_4g(H, under) && reaches_4g(H, top) && reaches_4g(H, top / H + (H > 1)), "reaches_4g");
    // pitches whose height * pitch wraps 64 bits (from 2^64 / H, rounded up, to SIZE_MAX): no frame stride holds such a frame,
    // whatever the wrapped product let through
    for (size_t pitch : { top / H + (H > 1), top - (H > 1), top })
      for (size_t stride : { fs, pitch * H, (size_t)0, top - 1 }) {
        if (H == 1 && stride >= pitch) continue;  // (one row: height * pitch is the pitch, and such a stride holds it)
        VCHECK(rule(base, pitch, stride, 2) == VIEW_STRIDE, "%s: wrapping pitch %zx, stride %zx, n = 2", s.entry, pitch, stride);
        VCHECK(rule(base, pitch, stride, 1) == (s.align == 2 && ((pitch | stride) & 1) ? VIEW_ALIGN : far), "%s: wrapping pitch %zx, stride %zx, n = 1", s.entry, pitch, stride);
      }
  }
}

// chunks of `rows` rows cover H, the last one is not empty
static bool chunks_cover(int nchunks, int rows, int H) { return rows >= 1 && (long)nchunks * rows >= H && (long)(nchunks - 1) * rows < H; }
static int largest_power_dividing(uintptr_t bits) { return bits % 8 == 0 ? 8 : bits % 4 == 0 ? 4 : 2; }

static void call_plans(int W, int H, int C, int max_batch)
{
  const int k = 7 * W + 3 * H + C;  // (every residue of address, pitch and frame stride comes by over the sweep)
  const size_t ip = (size_t)W * C + (k & 3), ifs = ip * H + ((k >> 2) & 3), op = (size_t)2 * W * C + 2 * ((k >> 4) & 3), ofs = op * H + 2 * ((k >> 6) & 3);
  const View in{ 0x10000000u + ((unsigned)(k >> 8) & 3), ip, ifs }, dx{ 0x20000000u + 2 * ((unsigned)(k >> 10) & 3), op, ofs };
  const uintptr_t dy = 0x30000000u + 2 * ((unsigned)(k >> 12) & 3);
  for (int n : { 1, std::min(2, max_batch), max_batch }) {
    const DerivPlan D = plan_derivatives(W, H, C, in, dx, dy, n, 3);
    const DerivParams &d = D.dp;
    VCHECK(!D.error && chunks_cover(d.nchunks, DERIV_CHUNK_ROWS, H) && (long)d.nstrips * DERIV_STRIP_W >= W && (long)(d.nstrips - 1) * DERIV_STRIP_W < W
           && d.total_items == n * d.nstrips * d.nchunks, "derivatives %d x %d x %d n %d: strips, chunks, items", W, H, C, n);
    VCHECK(d.out_align == largest_power_dividing(dx.p | dy | op | ofs) && (d.in_aligned != 0) == (in.p % 4 == 0 && ip % 4 == 0 && ifs % 4 == 0), "derivatives %d x %d x %d: alignments", W, H, C);
    VCHECK(d.in == (const uint8_t *)in.p && d.in_pitch == ip && d.in_frame_stride == ifs && d.dx == (uint8_t *)dx.p && d.dy == (uint8_t *)dy && d.pitch == op && d.frame_stride == ofs
           && d.W == W && d.H == H && d.nframes == n && d.channels == C && d.ksize == 3, "derivatives %d x %d x %d n %d: views", W, H, C, n);
    const HistParams h = plan_histogram(W, H, C, in, n);
    VCHECK(chunks_cover(h.nchunks, h.chunk_rows, H) && h.chunk_rows <= HIST_MAX_CHUNK_ROWS && h.total_items == n * h.nchunks && h.row_bytes == W * C && h.H == H && h.nframes == n
           && h.in == (const uint8_t *)in.p && h.in_pitch == ip && h.in_frame_stride == ifs && h.hist == nullptr, "histogram %d x %d x %d n %d", W, H, C, n);
  }
  // the maps of a run: one per frame, three with HC_OPT_PER_CHANNEL; the table of per-item counts holds any batch of them
  const View map{ 0x40000000u + ((unsigned)k & 7), (size_t)W + (k & 3), ((size_t)W + (k & 3)) * H + ((k >> 2) & 7) };
  for (int per_channel = 0; per_channel <= (C == 3); ++per_channel)
    for (int n : { 1, std::min(2, max_batch), max_batch * (per_channel ? 3 : 1) }) {  // (every n the entry lets through)
      const EdgePlan E = plan_edge_points(W, H, C, max_batch, map, n, 0x50000000u, 0x60000000u, 100);
      const EdgePointsParams &e = E.ep;
      VCHECK(!E.error && chunks_cover(e.nchunks, e.chunk_rows, H) && e.total_items == n * e.nchunks && (size_t)e.total_items <= E.table_items && e.items == nullptr,
             "edge points %d x %d x %d n %d of %d: chunks, items, table of %zu", W, H, C, n, max_batch, E.table_items);
      VCHECK(e.map == (const uint8_t *)map.p && e.pitch == map.pitch && e.frame_stride == map.fs && e.counts == (u32 *)0x50000000u && e.points == (int32_t *)0x60000000u && e.capacity == 100
             && e.W == W && e.H == H && e.nframes == n, "edge points %d x %d x %d n %d: views", W, H, C, n);
    }
}

// Plans worked out by hand from the expressions of the commit before these functions, where hc_derivatives_device, queue_histogram and
// hc_edge_points_device formed them inline: nstrips = ceil(W / 248), nchunks = ceil(H / 64), total_items = n * nstrips * nchunks
// (derivatives); chunk_rows = min(H, clamp(ceil(H * n / 8192), 8, 64)), nchunks = ceil(H / chunk_rows), total_items = n * nchunks
// (histogram, edge points); table_items = max_batch * (C == 3 ? 3 : 1) * ceil(H / min(8, H)).
static void pinned_call_plans()
{
  const struct { int W, H, C, max_batch, n; int d_strips, d_chunks, d_items, rows, chunks, items; size_t table; } pins[] = {
    { 64, 32, 3, 2, 2, 1, 1, 2, 8, 4, 8, 24 },  // test_gpu_derivatives.py::test_errors; H * n = 64 rows: the 8-row floor
    { 1920, 1080, 1, 1024, 1024, 8, 17, 139264, 64, 17, 17408, 138240 },  // 1 105 920 rows / 8192 = 135: the 64-row cap; 135 chunks of 8 rows
    { 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1 },
  };
  for (const auto &p : pins) {
    const View in{ 0x10000000u, (size_t)p.W * p.C, (size_t)p.W * p.C * p.H }, dx{ 0x20000000u, 2 * in.pitch, 2 * in.fs }, map{ 0x40000000u, (size_t)p.W, (size_t)p.W * p.H };
    const DerivPlan D = plan_derivatives(p.W, p.H, p.C, in, dx, 0x30000000u, p.n, 5);
    VCHECK(!D.error && D.dp.nstrips == p.d_strips && D.dp.nchunks == p.d_chunks && D.dp.total_items == p.d_items && D.dp.in_aligned == (in.pitch % 4 == 0) && D.dp.out_align == (in.pitch % 4 == 0 ? 8 : in.pitch % 2 == 0 ? 4 : 2),
           "pinned derivatives %d x %d: %d strips x %d chunks, %d items", p.W, p.H, D.dp.nstrips, D.dp.nchunks, D.dp.total_items);
    const HistParams h = plan_histogram(p.W, p.H, p.C, in, p.n);
    VCHECK(h.chunk_rows == p.rows && h.nchunks == p.chunks && h.total_items == p.items && h.row_bytes == p.W * p.C, "pinned histogram %d x %d: %d rows x %d, %d items", p.W, p.H, h.chunk_rows, h.nchunks, h.total_items);
    const EdgePlan E = plan_edge_points(p.W, p.H, p.C, p.max_batch, map, p.n, 0x50000000u, 0, 0);
    VCHECK(!E.error && E.ep.chunk_rows == p.rows && E.ep.nchunks == p.chunks && E.ep.total_items == p.items && E.table_items == p.table, "pinned edge points %d x %d: %d rows x %d, %d items, table %zu", p.W, p.H,
           E.ep.chunk_rows, E.ep.nchunks, E.ep.total_items, E.table_items);
  }
  // the refusals: work items beyond an int, a list buffer beyond size_t
  const View v{ 0x10000000u, 8184, (size_t)8184 << 24 };
  VCHECK(plan_derivatives(8184, 1 << 24, 1, v, v, 0x30000000u, 1 << 20, 3).error && !plan_derivatives(8184, 1 << 24, 1, v, v, 0x30000000u, 1, 3).error, "derivatives: too many work items");
  VCHECK(plan_edge_points(64, 1 << 24, 1, 1 << 30, v, 1, 4, 8, 1).error && plan_edge_points(64, 1 << 24, 1, 1 << 30, v, 1 << 30, 4, 8, 1).error && !plan_edge_points(64, 1 << 24, 1, 1 << 9, v, 1 << 9, 4, 8, 1).error,
         "edge points: too many work items / table entries");
  VCHECK(plan_edge_points(16, 8, 1, 2, v, 2, 4, 8, SIZE_MAX / 16 + 1).error && !plan_edge_points(16, 8, 1, 2, v, 2, 4, 8, SIZE_MAX / 16).error && plan_edge_points(16, 8, 1, 2, v, 1, 4, 8, SIZE_MAX / 8 + 1).error,
         "edge points: capacity * 8 * nframes");
}

static void views_and_call_plans()
{
  for (int H : { 1, 2, 32, 37, 1080, 4320 })
    for (int W : { 1, 16, 64, 641, 1920 })
      for (int C : { 1, 3 }) view_table(W, H, C);
  for (int W = 1; W <= 600; ++W)
    for (int H = 1; H <= 300; ++H)
      for (int C : { 1, 3 }) call_plans(W, H, C, 1 + (W + 5 * H) % 11);
  pinned_call_plans();
}

int main()
{
  const int heights[] = { 1, 8, 480, 1080, 4320 };  // every width at these heights, every height at these widths; the full option product where both are special
  const int widths[] = { 1, 8, 240, 248, 496, 640, 1920, 3840, 8184 };
  const int special[] = { 1, 7, 8, 16, 239, 240, 241, 247, 248, 249, 480, 495, 496, 497, 1079, 1080, 2160, 4320 };
  auto is_special = [&](int v) { for (int s : special) if (s == v) return true; return false; };
  for (int H : heights)
    for (int W = 1; W <= 8184; ++W) sweep_geometry(W, H, is_special(W) && is_special(H));
  for (int W : widths)
    for (int H = 1; H <= 4400; ++H) sweep_geometry(W, H, is_special(W) && is_special(H));
  for (int W : special)
    for (int H : special) sweep_geometry(W, H, true);
  pinned();
  pinned_front8_runs();
  chain_watch();
  views_and_call_plans();
  if (plane_row_dwords(8184) != 256 || plane_row_dwords(8185) != 0) { ++g_fail; std::printf("FAIL width limit\n"); }
  if (g_fail) { std::printf("%ld violations in %ld plans\n", g_fail, g_plans); return 1; }
  std::printf("ok %ld %016llx\n", g_plans, g_digest);
  return 0;
}
