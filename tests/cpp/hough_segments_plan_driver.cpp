// hough_segments_plan_driver.cpp -- plan_hough_segments, seg_on_scratch and hough_walk_tables of cudacam_amd/csrc/host_plan.h,
// checked without a GPU (tests/test_hough_segments_plan_cpu.py builds this with g++ under ASan + UBSan): every refusal
// hc_hough_segments_device documents, scratch sizes, grids and scratch pointers at their boundaries, and that a refused plan holds
// nothing.  Prints "ok <checks>" or the first violations.
//   hough_segments_plan_driver tables W H rho theta min_theta max_theta     (the doubles as C99 hex floats)
// prints "numangle" and one line per angle: major and the bits of slope and scale as hex words.
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

using namespace hc;

static long g_checks = 0, g_fail = 0;
#define VCHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL "); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const double PI = HOUGH_PI, DEG = HOUGH_PI / 180;
static const uintptr_t MAP = 0x10000001u, LN = 0x20000000u, LC = 0x30000000u, SC = 0x40000000u, SG = 0x50000000u;  // (the map at an odd address)
static const double INF = std::numeric_limits<double>::infinity(), NaN = std::numeric_limits<double>::quiet_NaN();

struct Call {
  int W = 64, H = 48, max_frames = 4, n = 2;
  View map{ MAP, 67, 67 * 48 + 5 };
  uintptr_t lines = LN, line_counts = LC, seg_counts = SC, segs = SG;
  size_t lcap = 16, scap = 100;
  double rho = 1, theta = DEG, lo = 0, hi = PI;
  int min_length = 10, max_gap = 2;
  SegPlan plan() const { return plan_hough_segments(W, H, max_frames, map, lines, line_counts, lcap, n, rho, theta, lo, hi, min_length, max_gap, seg_counts, segs, scap); }
};

static bool holds_nothing(const SegPlan &P)
{
  const SegPlan Z;
  return P.error && P.items_bytes == 0 && P.table_bytes == 0 && P.lines_grid == 0 && P.scan_grid == 0 && !P.emit && std::memcmp(&P.sp, &Z.sp, sizeof P.sp) == 0;
}
#define REFUSED(call, ...) do { const SegPlan R_ = (call).plan(); VCHECK(holds_nothing(R_), __VA_ARGS__); } while (0)
#define TAKEN(call, ...) do { const SegPlan R_ = (call).plan(); VCHECK(!R_.error, __VA_ARGS__); } while (0)

static void refusals()
{
  TAKEN(Call(), "the valid call");
  { Call c; c.map.p = 0; REFUSED(c, "d_map null"); }
  { Call c; c.lines = 0; REFUSED(c, "d_lines null"); }
  { Call c; c.line_counts = 0; REFUSED(c, "d_line_counts null"); }
  { Call c; c.seg_counts = 0; REFUSED(c, "d_seg_counts null"); }
  { Call c; c.segs = 0; REFUSED(c, "d_segs null with seg_capacity > 0"); }
  { Call c; c.segs = 0; c.scap = 0; TAKEN(c, "d_segs null with seg_capacity 0"); }
  { Call c; c.scap = 0; TAKEN(c, "d_segs given with seg_capacity 0"); }
  for (unsigned o = 1; o < 4; ++o) {
    { Call c; c.lines += o; REFUSED(c, "d_lines + %u", o); }
    { Call c; c.line_counts += o; REFUSED(c, "d_line_counts + %u", o); }
    { Call c; c.seg_counts += o; REFUSED(c, "d_seg_counts + %u", o); }
  }
  for (unsigned o = 1; o < 16; ++o) {
    Call c; c.segs += o; REFUSED(c, "d_segs + %u", o);
    c.scap = 0; REFUSED(c, "d_segs + %u with seg_capacity 0", o);
  }
  { Call c; c.min_length = -1; REFUSED(c, "min_length -1"); }
  { Call c; c.max_gap = -1; REFUSED(c, "max_gap -1"); }
  { Call c; c.min_length = 0; c.max_gap = 0; TAKEN(c, "min_length and max_gap 0"); }
  { Call c; c.min_length = 0x7FFFFFFF; c.max_gap = 0x7FFFFFFF; TAKEN(c, "min_length and max_gap INT_MAX"); }
  for (int n : { 0, -1, 5, 1 << 30 }) { Call c; c.n = n; REFUSED(c, "nframes %d of 4", n); }
  { Call c; c.n = 4; c.map.fs = 67 * 48; TAKEN(c, "nframes = max, the smallest frame stride"); }
  // the view: as hc_edge_points_device
  { Call c; c.map.pitch = 63; REFUSED(c, "a pitch below the width"); }
  { Call c; c.map.pitch = 64; c.map.fs = 64 * 48; TAKEN(c, "a tight view"); }
  { Call c; c.map.fs = 67 * 48 - 1; REFUSED(c, "a frame stride below height * pitch"); }
  { Call c; c.n = 1; c.map.fs = 0; TAKEN(c, "one frame: any frame stride"); }
  { Call c; c.n = 1; c.map.pitch = ((size_t)1 << 32) / 48 + 1; REFUSED(c, "height * pitch >= 2^32"); }
  { Call c; c.n = 1; c.map.pitch = 0xFFFFFFFFull / 48; TAKEN(c, "height * pitch just below 2^32"); }
  { Call c; c.n = 1; c.map.pitch = SIZE_MAX; REFUSED(c, "a pitch that would wrap"); }
  // the geometry: as hc_hough_lines_device
  for (double v : { 0.0, -1.0, INF, -INF, NaN }) {
    { Call c; c.rho = v; REFUSED(c, "rho %g", v); }
    { Call c; c.theta = v; REFUSED(c, "theta %g", v); }
  }
  for (double v : { INF, -INF, NaN }) {
    { Call c; c.lo = v; REFUSED(c, "min_theta %g", v); }
    { Call c; c.hi = v; REFUSED(c, "max_theta %g", v); }
  }
  { Call c; c.lo = 1.0; c.hi = 0.5; REFUSED(c, "max_theta < min_theta"); }
  { Call c; c.lo = 1.0; c.hi = 1.0; const SegPlan P = c.plan(); VCHECK(!P.error && P.sp.numangle == 1 && P.table_bytes == 16, "max_theta == min_theta: one angle"); }
  { Call c; c.rho = 1e-6; REFUSED(c, "a tiny rho: an accumulator row beyond LDS"); }
  { Call c; c.W = 1; c.H = 1; c.map.pitch = 1; c.map.fs = 1; c.theta = 1e-9; REFUSED(c, "(numangle + 2) * (numrho + 2) >= 2^31"); }
  { Call c; c.W = 0; REFUSED(c, "width 0"); }
  // capacities
  { Call c; c.lcap = 0; REFUSED(c, "line_capacity 0"); }
  { Call c; c.lcap = SIZE_MAX / 12 / 2 + 1; REFUSED(c, "line_capacity * 12 * nframes overflows"); }
  { Call c; c.lcap = SIZE_MAX / 4 / 2 + 1; REFUSED(c, "line_capacity * 4 * nframes overflows"); }
  { Call c; c.scap = SIZE_MAX / 16 / 2 + 1; REFUSED(c, "seg_capacity * 16 * nframes overflows"); }
  { Call c; c.scap = SIZE_MAX / 16 / 2; TAKEN(c, "the largest seg_capacity"); }
  { Call c; c.lcap = (size_t)0x7FFFFFF0 / 2 + 1; REFUSED(c, "nframes * line_capacity above 2^31 - 16"); }
  { Call c; c.lcap = (size_t)0x7FFFFFF0 / 2; REFUSED(c, "64 x 48: 2^30 - 8 lines of up to 32 segments reach 2^32"); }
  { Call c; c.lcap = 0xFFFFFFFFu / 32; const SegPlan P = c.plan(); VCHECK(!P.error && P.sp.total_items == (int)(2 * (0xFFFFFFFFu / 32)), "the most lines whose segments a uint32 counts"); }
  { Call c; c.lcap = 0xFFFFFFFFu / 32 + 1; REFUSED(c, "one line more"); }
  { Call c; c.W = 1; c.H = 1; c.n = 1; c.map.pitch = 1; c.lcap = 0x7FFFFFF0; const SegPlan P = c.plan(); VCHECK(!P.error && P.sp.total_items == 0x7FFFFFF0 && P.lines_grid == 0x7FFFFFF0 / 4, "1 x 1: 2^31 - 16 line slots"); }
  { Call c; c.W = 1; c.H = 1; c.n = 1; c.map.pitch = 1; c.lcap = 0x7FFFFFF1; REFUSED(c, "1 x 1: a line slot more"); }
}

static void shapes()
{
  for (int n : { 1, 2, 3, 4, 5, 8, 9, 1024 })
    for (size_t lcap : { (size_t)1, (size_t)2, (size_t)3, (size_t)4, (size_t)5, (size_t)63, (size_t)64, (size_t)65, (size_t)1000 })
      for (size_t scap : { (size_t)0, (size_t)1, (size_t)77 }) {
        Call c; c.W = 1920; c.H = 1080; c.max_frames = 1024; c.n = n; c.lcap = lcap; c.scap = scap; c.map = View{ MAP, 1921, (size_t)1921 * 1080 + 3 };
        const SegPlan P = c.plan();
        const size_t items = (size_t)n * lcap;
        VCHECK(!P.error && P.sp.numangle == 180 && P.table_bytes == 180 * 16 && P.items_bytes == items * 4 && P.sp.total_items == (int)items, "1080p n %d lcap %zu: scratch", n, lcap);
        VCHECK(P.lines_grid == (unsigned)((items + 3) / 4) && (size_t)P.lines_grid * 4 >= items && ((size_t)P.lines_grid - 1) * 4 < items && P.scan_grid == (unsigned)((n + 3) / 4) && P.emit == (scap > 0),
               "1080p n %d lcap %zu scap %zu: grids %u %u", n, lcap, scap, P.lines_grid, P.scan_grid);
        VCHECK((uintptr_t)P.sp.map == MAP && P.sp.pitch == 1921 && P.sp.frame_stride == (size_t)1921 * 1080 + 3 && (uintptr_t)P.sp.lines == LN && (uintptr_t)P.sp.line_counts == LC && P.sp.line_capacity == lcap
               && (uintptr_t)P.sp.seg_counts == SC && (uintptr_t)P.sp.segs == SG && P.sp.seg_capacity == scap && P.sp.W == 1920 && P.sp.H == 1080 && P.sp.nframes == n && P.sp.min_length == 10 && P.sp.max_gap == 2,
               "1080p n %d: the caller's arguments", n);
        VCHECK(!P.sp.items && !P.sp.tab_theta && !P.sp.tab_major && !P.sp.tab_slope && !P.sp.tab_scale, "the plan holds no scratch pointer");
        const uintptr_t I = 0x70000000u, T = 0x60000000u;
        const SegParams s = seg_on_scratch(P, I, T);
        VCHECK((uintptr_t)s.items == I && (uintptr_t)s.tab_theta == T && (uintptr_t)s.tab_major == T + 4 * 180 && (uintptr_t)s.tab_slope == T + 8 * 180 && (uintptr_t)s.tab_scale == T + 12 * 180
               && (uintptr_t)s.tab_scale + 4 * 180 == T + P.table_bytes && s.total_items == P.sp.total_items && s.seg_capacity == scap, "scratch pointers");
      }
  { Call c; c.theta = PI / 4; const SegPlan P = c.plan(); VCHECK(!P.error && P.sp.numangle == 4 && P.table_bytes == 64, "four angles"); }
}

static void table_refusals()
{
  int32_t mj[8];
  float sl[8], sc[8];
  for (int i = 0; i < 8; ++i) { mj[i] = -77; sl[i] = sc[i] = -77.0f; }
  int a = -7;
  auto clean = [&]() {
    bool ok = a == -7;
    for (int i = 0; i < 8; ++i) ok = ok && mj[i] == -77 && sl[i] == -77.0f && sc[i] == -77.0f;
    return ok;
  };
  VCHECK(hough_walk_tables(64, 48, 1, PI / 4, 0, PI, nullptr, mj, sl, sc, 8) && clean(), "numangle null");
  VCHECK(hough_walk_tables(64, 48, 1, PI / 4, 0, PI, &a, mj, nullptr, sc, 8) && hough_walk_tables(64, 48, 1, PI / 4, 0, PI, &a, nullptr, nullptr, sc, 8) && hough_walk_tables(64, 48, 1, PI / 4, 0, PI, &a, nullptr, sl, sc, 8)
         && clean(), "some tables only");
  VCHECK(hough_walk_tables(64, 48, 1, PI / 4, 0, PI, &a, mj, sl, sc, 3) && clean(), "table_capacity 3 < numangle 4");
  VCHECK(hough_walk_tables(64, 48, 0, PI / 4, 0, PI, &a, mj, sl, sc, 8) && hough_walk_tables(64, 48, 1, NaN, 0, PI, &a, mj, sl, sc, 8) && hough_walk_tables(64, 48, 1, 1, 2, 1, &a, mj, sl, sc, 8)
         && hough_walk_tables(0, 48, 1, 1, 0, PI, &a, mj, sl, sc, 8) && clean(), "geometry refusals");
  VCHECK(!hough_walk_tables(64, 48, 1, PI / 4, 0, PI, &a, nullptr, nullptr, nullptr, 0) && a == 4 && mj[0] == -77, "numangle only");
  VCHECK(!hough_walk_tables(64, 48, 1, PI / 4, 0, PI, &a, mj, sl, sc, 4) && mj[0] == 1 && sl[0] == 0.0f && sc[0] == 1.0f && mj[1] == 0 && mj[2] == 0 && mj[3] == 1 && mj[4] == -77 && sl[4] == -77.0f && sc[4] == -77.0f,
         "four angles, nothing behind them");
  float th[4] = { -77.0f, -77.0f, -77.0f, -77.0f };
  VCHECK(!hough_walk_tables(64, 48, 1, PI / 4, 0, PI, &a, mj, sl, sc, 4, th) && th[0] == 0.0f && th[1] == (float)(PI / 4) && th[2] == (float)(PI / 4) + (float)(PI / 4), "the angles beside the tables");
  for (int n = 0; n < 4; ++n) VCHECK(std::fabs(sl[n]) <= 1.0f, "|slope[%d]| = %g", n, sl[n]);
}

static int print_tables(char **v)
{
  const int W = std::atoi(v[0]), H = std::atoi(v[1]);
  const double rho = std::strtod(v[2], nullptr), theta = std::strtod(v[3], nullptr), lo = std::strtod(v[4], nullptr), hi = std::strtod(v[5], nullptr);
  int a = 0;
  if (const char *e = hough_walk_tables(W, H, rho, theta, lo, hi, &a, nullptr, nullptr, nullptr, 0)) { std::printf("refused: %s\n", e); return 1; }
  std::vector<int32_t> mj(a);
  std::vector<float> sl(a), sc(a);
  if (hough_walk_tables(W, H, rho, theta, lo, hi, &a, mj.data(), sl.data(), sc.data(), (size_t)a)) return 1;
  std::printf("%d\n", a);
  for (int n = 0; n < a; ++n) {
    uint32_t w[2];
    std::memcpy(&w[0], &sl[n], 4); std::memcpy(&w[1], &sc[n], 4);
    std::printf("%d %08x %08x\n", mj[n], w[0], w[1]);
  }
  return 0;
}

int main(int argc, char **argv)
{
  if (argc == 8 && !std::strcmp(argv[1], "tables")) return print_tables(argv + 2);
  refusals();
  shapes();
  table_refusals();
  if (g_fail) { std::printf("%ld of %ld checks failed\n", g_fail, g_checks); return 1; }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
