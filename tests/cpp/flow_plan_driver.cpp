// flow_plan_driver.cpp -- plan_pyr_down and plan_lk_flow of cudacam_amd/csrc/host_plan.h, checked without a GPU
// (tests/test_flow_plan_cpu.py builds this with g++ under ASan + UBSan): the level geometry, the strips / chunks and alignment flags
// of k_pyr_down8, the grid and round classes of k_lk_flow, and every refusal the two entries document, each beside its nearest
// neighbour that passes.
// Prints "ok <checks>" or the first violations.
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstring>
#include <limits>

using namespace hc;

static long g_checks = 0, g_fail = 0;
#define VCHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL "); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();

static void pyr_geometry()
{
  const int ws[] = { 3, 4, 5, 247, 248, 249, 496, 497, 1920 }, strips[] = { 1, 1, 1, 1, 1, 2, 2, 3, 8 }, dws[] = { 2, 2, 3, 124, 124, 125, 248, 249, 960 };
  const int hs[] = { 3, 4, 63, 64, 65, 129, 1080 }, chunks[] = { 1, 1, 1, 1, 2, 3, 17 }, dhs[] = { 2, 2, 32, 32, 33, 65, 540 };
  for (int i = 0; i < 9; ++i)
    for (int j = 0; j < 7; ++j)
      for (int n : { 1, 3 })
        for (int bits = 0; bits < 64; ++bits) {
          const int W = ws[i], H = hs[j];
          const size_t ip = round_up((size_t)W, 4) + 4 + ((bits >> 2) & 3), op = round_up((size_t)dws[i], 2) + 2 + ((bits >> 4) & 1);
          const View src{ 0x10000000u + (bits & 3), ip, round_up(ip * H, 4) + ((bits >> 1) & 3) }, dst{ 0x60000000u + ((bits >> 5) & 1), op, round_up(op * dhs[j], 2) + ((bits >> 3) & 1) };
          const PyrPlan P = plan_pyr_down(1920, 1080, 4, src, W, H, dst, n);
          VCHECK(!P.error, "%d x %d bits %x: %s", W, H, bits, P.error ? P.error : "");
          if (P.error) continue;
          const PyrParams &q = P.pp;
          VCHECK(q.dW == dws[i] && q.dH == dhs[j] && q.W == W && q.H == H && q.nframes == n, "%d x %d: level %d x %d", W, H, q.dW, q.dH);
          VCHECK(q.nstrips == strips[i] && q.nchunks == chunks[j] && q.total_items == n * strips[i] * chunks[j], "%d x %d: %d strips %d chunks", W, H, q.nstrips, q.nchunks);
          VCHECK(q.in_aligned == (((src.p | src.pitch | src.fs) & 3) == 0) && q.out_aligned == (((dst.p | dst.pitch | dst.fs) & 1) == 0), "%d x %d bits %x: alignment flags", W, H, bits);
          VCHECK(q.in == (const uint8_t *)src.p && q.out == (uint8_t *)dst.p && q.in_pitch == ip && q.in_frame_stride == src.fs && q.out_pitch == op && q.out_frame_stride == dst.fs, "%d x %d: the block", W, H);
        }
  const PyrPlan P = plan_pyr_down(1920, 1080, 64, View{ 0x10000000u, 1920, 1920 * 1080 }, 1920, 1080, View{ 0x60000000u, 960, 960 * 540 }, 64);
  VCHECK(!P.error && P.pp.total_items == 64 * 8 * 17 && P.pp.in_aligned && P.pp.out_aligned && P.pp.dW == 960 && P.pp.dH == 540, "pinned 1080p x 64");
  // the chain of levels of a 130 x 70 frame: every level is no larger than the frame
  int w = 130, h = 70;
  const int want[][2] = { { 65, 35 }, { 33, 18 }, { 17, 9 }, { 9, 5 }, { 5, 3 } };
  for (int l = 0; l < 5; ++l) {
    const PyrPlan L = plan_pyr_down(130, 70, 1, View{ 0x1000, (size_t)w, 0 }, w, h, View{ 0x9000, (size_t)pyr_half(w), 0 }, 1);
    VCHECK(!L.error && L.pp.dW == want[l][0] && L.pp.dH == want[l][1], "level %d of 130 x 70", l + 1);
    w = pyr_half(w); h = pyr_half(h);
  }
}

static void pyr_refusals()
{
  constexpr int W = 70, H = 32, dw = 35, dh = 16;
  const View src{ 0x10000000u, 72, 72 * 32 }, dst{ 0x60000000u, 36, 36 * 16 };
  auto plan = [&](const View &s, const View &d, int n = 2, int sw = 70, int sh = 32, int mf = 4) { return plan_pyr_down(W, H, mf, s, sw, sh, d, n); };
  auto refused = [](const PyrPlan &P, const char *text) { return P.error && std::strstr(P.error, text) && !P.pp.in && !P.pp.out && !P.pp.total_items; };
  VCHECK(!plan(src, dst).error && !plan(src, dst, 4).error && !plan(src, dst, 1, 3, 3).error, "the valid calls");
  VCHECK(refused(plan(View{ 0, 72, 72 * 32 }, dst), "null") && refused(plan(src, View{ 0, 36, 36 * 16 }), "null"), "null pointers");
  for (int s : { -1, 0, 1, 2 }) VCHECK(refused(plan(src, dst, 2, s, H), "3 at least") && refused(plan(src, dst, 2, W, s), "3 at least"), "side %d", s);
  VCHECK(refused(plan(src, dst, 2, W + 1, H), "exceed") && refused(plan(src, dst, 2, W, H + 1), "exceed") && !plan(src, dst, 2, W - 1, H - 1).error, "levels no larger than the frame");
  VCHECK(refused(plan(src, dst, 0), "nframes") && refused(plan(src, dst, -1), "nframes") && refused(plan(src, dst, 5), "nframes") && !plan(src, dst, 5, W, H, 5).error, "nframes within 1 .. the bound");
  VCHECK(refused(plan(View{ src.p, W - 1, 72 * 32 }, dst), "pitch smaller") && !plan(View{ src.p, W, W * H }, dst).error, "pitch below / equal to a source row");
  VCHECK(refused(plan(src, View{ dst.p, dw - 1, 36 * 16 }), "dst_pitch") && !plan(src, View{ dst.p, dw, dw * dh }).error, "dst_pitch below / equal to a destination row");
  VCHECK(refused(plan(View{ src.p, 72, 72 * 32 - 1 }, dst, 2), "frame stride") && !plan(View{ src.p, 72, 72 * 32 - 1 }, dst, 1).error, "a source frame stride below height * pitch at n = 2, not at n = 1");
  VCHECK(refused(plan(src, View{ dst.p, 36, 36 * 16 - 1 }, 2), "dst_frame_stride") && !plan(src, View{ dst.p, 36, 36 * 16 - 1 }, 1).error && !plan(src, View{ dst.p, 36, 36 * 16 }, 2).error,
         "a destination frame stride below dh * dst_pitch (the level's height, not the frame's)");
  const size_t huge = ((size_t)1 << 32) / H, hugd = ((size_t)1 << 32) / dh;
  VCHECK(refused(plan(View{ src.p, huge, huge * H }, View{ 0x600000000000ull, 36, 36 * 16 }, 1), "2^32") && refused(plan(src, View{ 0x600000000000ull, hugd, hugd * dh }, 1), "2^32")
         && !plan(View{ src.p, huge - 1, 0 }, View{ 0x600000000000ull, hugd - 1, 0 }, 1).error, "height * pitch >= 2^32 on either side");
  VCHECK(refused(plan(View{ UINTPTR_MAX - 100, 72, 72 * 32 }, dst, 1), "wraps") && refused(plan(src, View{ UINTPTR_MAX - 100, 36, 36 * 16 }, 1), "wraps"), "views that wrap the address space");
  const size_t in2 = 72 * 32 + 31 * 72 + W, out2 = 36 * 16 + 15 * 36 + dw;  // the byte ranges of two frames
  VCHECK(refused(plan(src, View{ src.p, 36, 36 * 16 }), "overlap"), "in place");
  VCHECK(refused(plan(src, View{ src.p + in2 - 1, 36, 36 * 16 }), "overlap") && !plan(src, View{ src.p + in2, 36, 36 * 16 }).error, "the destination begins on / behind the source's last byte");
  VCHECK(refused(plan(src, View{ src.p - out2 + 1, 36, 36 * 16 }), "overlap") && !plan(src, View{ src.p - out2, 36, 36 * 16 }).error, "the destination ends on / before the source's first byte");
}

struct FlowCall {
  View prev{ 0x10000000u, 100, 100 * 61 };
  uintptr_t next = 0x20000000u, counts = 0x30000000u, prev_pts = 0x40000000u, next_pts = 0x50000000u, status = 0x60000000u, err = 0x70000000u;
  int w = 97, h = 61, level = 0, n = 2, win = 21, iters = 30, use_initial = 0, max_frames = 4;
  size_t capacity = 100;
  double eps = 0.01, min_eig = 1e-4;
  FlowPlan plan() const { return plan_lk_flow(97, 61, max_frames, prev, next, w, h, level, n, counts, prev_pts, next_pts, capacity, win, iters, eps, min_eig, use_initial, status, err); }
};

static void flow_geometry()
{
  const int cls[] = { 1, 1, 2, 2, 4, 4, 7, 7, 7, 10, 10, 16, 16, 16 };  // win = 5, 7, .., 31
  for (int win = 5, k = 0; win <= 31; win += 2, ++k) {
    VCHECK(flow_win_ok(win) && flow_round_class(win) == cls[k] && flow_rounds(win) <= cls[k] && 64 * flow_rounds(win) >= win * win && 64 * (flow_rounds(win) - 1) < win * win,
           "win %d: %d rounds, class %d", win, flow_rounds(win), flow_round_class(win));
    for (size_t cap : { (size_t)1, (size_t)3, (size_t)4, (size_t)5, (size_t)1024, (size_t)1 << 30 }) {
      FlowCall c; c.win = win; c.capacity = cap; c.n = 1; c.prev_pts = 0x100000000000ull; c.next_pts = 0x300000000000ull;
      const FlowPlan P = c.plan();
      VCHECK(!P.error && P.fp.groups == (u32)((cap + 3) / 4) && P.fp.capacity == cap && P.fp.win == win, "win %d capacity %zu: %s", win, cap, P.error ? P.error : "");
    }
  }
  VCHECK(flow_rounds(5) == 1 && flow_rounds(21) == 7 && 441 - 6 * 64 == 57 && flow_rounds(31) == 16 && 961 - 15 * 64 == 1, "25 pixels leave lanes idle, 441 = 6 rounds + 57, 961 = 15 rounds + 1");
  FlowCall c; c.eps = 0.03; c.min_eig = 0.001; c.use_initial = 7; c.level = 3;
  const FlowPlan P = c.plan();
  const FlowParams &f = P.fp;
  VCHECK(!P.error && f.eps2 == (float)(0.03 * 0.03) && f.min_eig == (float)0.001 && f.use_initial == 1 && f.level == 3 && f.W == 97 && f.H == 61 && f.nframes == 2 && f.max_iterations == 30,
         "the scalars as the kernel receives them");
  VCHECK(f.prev == (const uint8_t *)c.prev.p && f.next == (const uint8_t *)c.next && f.pitch == 100 && f.frame_stride == 6100 && f.counts == (const u32 *)c.counts && f.prev_pts == (const float *)c.prev_pts
         && f.next_pts == (float *)c.next_pts && f.status == (uint8_t *)c.status && f.err == (float *)c.err, "the pointers");
  FlowCall d; d.err = 0;
  VCHECK(!d.plan().error && d.plan().fp.err == nullptr, "d_err may be null");
  FlowCall e; e.w = 1; e.h = 1; e.prev = View{ 0x10000000u, 1, 1 };
  VCHECK(!e.plan().error, "a level of 1 x 1");
}

static void flow_refusals()
{
  auto refused = [](const FlowPlan &P, const char *text) { return P.error && std::strstr(P.error, text) && !P.fp.prev && !P.fp.next_pts && !P.fp.groups; };
  VCHECK(!FlowCall().plan().error, "the valid call");
#define WITH(stmt) [&] { FlowCall c; stmt; return c.plan(); }()
  VCHECK(refused(WITH(c.prev.p = 0), "null") && refused(WITH(c.next = 0), "null") && refused(WITH(c.counts = 0), "null") && refused(WITH(c.prev_pts = 0), "null")
         && refused(WITH(c.next_pts = 0), "null") && refused(WITH(c.status = 0), "null"), "null pointers");
  VCHECK(refused(WITH(c.counts += 2), "4-byte") && refused(WITH(c.prev_pts += 1), "4-byte") && refused(WITH(c.next_pts += 2), "4-byte") && refused(WITH(c.err += 3), "4-byte")
         && !WITH(c.counts += 4; c.prev_pts += 4; c.next_pts += 4; c.err += 4; c.status += 1).error, "point arrays 4-byte aligned, the status any");
  for (int l : { -1, 16, 100 }) VCHECK(refused(WITH(c.level = l), "level"), "level %d", l);
  for (int l : { 0, 15 }) VCHECK(!WITH(c.level = l).error, "level %d", l);
  for (int w : { -1, 0, 3, 4, 6, 20, 32, 33 }) VCHECK(refused(WITH(c.win = w), "win"), "win %d", w);
  for (int i : { -1, 0, 65 }) VCHECK(refused(WITH(c.iters = i), "max_iterations"), "max_iterations %d", i);
  for (int i : { 1, 64 }) VCHECK(!WITH(c.iters = i).error, "max_iterations %d", i);
  for (double v : { NaN, INF, -INF, -1e-300 }) VCHECK(refused(WITH(c.eps = v), "epsilon") && refused(WITH(c.min_eig = v), "min_eig_threshold"), "epsilon / min_eig_threshold %g", v);
  VCHECK(!WITH(c.eps = 0; c.min_eig = 0).error && !WITH(c.eps = 1e300).error, "zero and huge thresholds pass");
  VCHECK(refused(WITH(c.w = 0), "positive") && refused(WITH(c.h = 0), "positive") && refused(WITH(c.w = 98), "exceed") && refused(WITH(c.h = 62), "exceed"), "the level's size");
  VCHECK(refused(WITH(c.n = 0), "nframes") && refused(WITH(c.n = 5), "nframes") && !WITH(c.n = 4).error, "nframes within 1 .. the bound");
  VCHECK(refused(WITH(c.capacity = 0), "capacity") && refused(WITH(c.capacity = SIZE_MAX / 8 / 2 + 1), "overflows") && refused(WITH(c.capacity = ((size_t)1 << 30) + 1; c.prev_pts = 0x100000000000ull; c.next_pts = 0x300000000000ull), "2^30"),
         "capacity 0, overflowing, above the grid");
  VCHECK(refused(WITH(c.prev.pitch = 96), "pitch smaller") && !WITH(c.prev.pitch = 97; c.prev.fs = 97 * 61).error, "pitch below / equal to a row");
  VCHECK(refused(WITH(c.prev.fs = 100 * 61 - 1), "frame stride") && !WITH(c.prev.fs = 100 * 61 - 1; c.n = 1).error, "a frame stride below height * pitch at n = 2, not at n = 1");
  const size_t huge = ((size_t)1 << 32) / 61 + 1;
  VCHECK(refused(WITH(c.n = 1; c.prev.pitch = huge; c.prev.p = 0x100000000000ull; c.next = 0x200000000000ull), "2^32"), "height * pitch >= 2^32");
  VCHECK(refused(WITH(c.n = 1; c.prev.p = UINTPTR_MAX - 100), "wraps") && refused(WITH(c.n = 1; c.next = UINTPTR_MAX - 100), "wraps") && refused(WITH(c.next_pts = UINTPTR_MAX - 103), "wraps")
         && refused(WITH(c.prev_pts = UINTPTR_MAX - 103), "wraps") && refused(WITH(c.counts = UINTPTR_MAX - 3), "wraps"), "ranges that wrap the address space");
  const size_t pts = 100 * 8 * 2, img = 100 * 61 + 60 * 100 + 97;
  VCHECK(refused(WITH(c.next_pts = c.prev_pts), "d_prev_pts") && refused(WITH(c.next_pts = c.prev_pts + pts - 4), "d_prev_pts") && !WITH(c.next_pts = c.prev_pts + pts).error
         && refused(WITH(c.next_pts = c.prev_pts - pts + 4), "d_prev_pts") && !WITH(c.next_pts = c.prev_pts - pts).error, "d_next_pts against d_prev_pts");
  VCHECK(refused(WITH(c.next_pts = c.counts + 4), "d_counts") && !WITH(c.next_pts = c.counts + 8).error && refused(WITH(c.next_pts = c.counts - pts + 4), "d_counts") && !WITH(c.next_pts = c.counts - pts).error,
         "d_next_pts against d_counts");
  VCHECK(refused(WITH(c.next_pts = c.prev.p + img - 1), "image") && !WITH(c.next_pts = c.prev.p + img + 3).error && refused(WITH(c.next_pts = c.next + img - 1), "image") && !WITH(c.next_pts = c.next + img + 3).error
         && refused(WITH(c.next_pts = c.next - pts + 4), "image") && !WITH(c.next_pts = c.next - pts).error, "d_next_pts against either image");
  VCHECK(!WITH(c.next = c.prev.p).error, "prev and next may be the same planes");
#undef WITH
}

int main()
{
  pyr_geometry();
  pyr_refusals();
  flow_geometry();
  flow_refusals();
  if (g_fail) { std::printf("%ld of %ld checks failed\n", g_fail, g_checks); return 1; }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
