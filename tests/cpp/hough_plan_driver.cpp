// hough_plan_driver.cpp -- plan_hough_lines, hough_pass, hough_geometry and hough_tables of cudacam_amd/csrc/host_plan.h, checked
// without a GPU (tests/test_hough_plan_cpu.py builds this with g++ under ASan + UBSan): every refusal hc_hough_lines_device
// documents, rows per workgroup, groups, passes and scratch at their boundaries, the pointers of every pass, and that a refused
// plan holds nothing.  Prints "ok <checks>" or the first violations.
//   hough_plan_driver tables W H rho theta min_theta max_theta     (the doubles as C99 hex floats)
// prints "numangle numrho" and one line per angle: the bits of tab_cos, tab_sin, tab_theta as hex words.
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
static const uintptr_t PTS = 0x10000000u, PC = 0x20000000u, LC = 0x30000000u, LN = 0x40000000u;
static const double INF = std::numeric_limits<double>::infinity(), NaN = std::numeric_limits<double>::quiet_NaN();

static HoughPlan plan(int W, int H, int n, double rho, double theta, size_t bound = HOUGH_SCRATCH_BYTES, size_t lcap = 16, size_t pcap = 1000, int max_frames = 1024,
                      int thr = 10, double lo = 0, double hi = PI)
{
  return plan_hough_lines(W, H, max_frames, PTS, PC, pcap, n, rho, theta, thr, lo, hi, LC, LN, lcap, bound);
}

static bool holds_nothing(const HoughPlan &P)
{
  const HoughPlan Z;
  return P.error && P.frames == 0 && P.frames_per_pass == 0 && P.passes == 0 && P.scratch_bytes == 0 && P.total_work == 0 && P.vote_grid == 0 && P.rows_grid == 0 && P.scan_grid == 0
         && P.rank_grid_x == 0 && P.rank_grid_y == 0 && P.frame_accum_bytes == 0 && P.frame_peaks_bytes == 0 && P.frame_items_bytes == 0 && std::memcmp(&P.hp, &Z.hp, sizeof P.hp) == 0;
}
#define REFUSED(expr, ...) do { const HoughPlan R_ = (expr); VCHECK(holds_nothing(R_), __VA_ARGS__); } while (0)

static void geometry()
{
  int a = -7, r = -7;
  VCHECK(!hough_geometry(1920, 1080, 1, DEG, 0, PI, &a, &r) && a == 180 && r == 6001, "1080p: %d %d", a, r);
  VCHECK(!hough_geometry(64, 48, 1, DEG, 0.3, 1.2, &a, &r) && a == 52 && r == 225, "64x48 [0.3, 1.2]: %d %d", a, r);
  VCHECK(!hough_geometry(64, 48, 1, PI / 4, 0, PI, &a, &r) && a == 4 && r == 225, "64x48 pi/4: %d %d", a, r);
  VCHECK(!hough_geometry(64, 48, 1, 4.0, 0, PI, &a, &r) && a == 1 && r == 225, "64x48 theta 4: %d %d", a, r);
  VCHECK(!hough_geometry(64, 48, 2, DEG, 0, PI, &a, &r) && r == 112, "half to even: 112.5 -> %d", r);
  VCHECK(!hough_geometry(1, 1, 1e9, DEG, 0, PI, &a, &r) && r == 0, "a huge rho: numrho %d", r);
  a = r = -7;
  VCHECK(hough_geometry(0, 48, 1, DEG, 0, PI, &a, &r) && hough_geometry(64, 0, 1, DEG, 0, PI, &a, &r) && a == -7 && r == -7, "an empty frame, nothing written");
}

static void refusals()
{
  VCHECK(!plan(64, 48, 2, 1, DEG).error, "the valid call");
  auto raw = [](uintptr_t pts, uintptr_t pc, uintptr_t lc, uintptr_t ln, size_t lcap, size_t pcap = 100, int n = 1) {
    return plan_hough_lines(64, 48, 4, pts, pc, pcap, n, 1, DEG, 10, 0, PI, lc, ln, lcap, HOUGH_SCRATCH_BYTES);
  };
  VCHECK(!raw(PTS, PC, LC, LN, 4).error && !raw(PTS, PC, LC, 0, 0).error && !raw(PTS, PC, LC, LN, 0).error, "valid pointer sets (d_lines may be null with line_capacity 0)");
  REFUSED(raw(0, PC, LC, LN, 4), "d_points null");
  REFUSED(raw(PTS, 0, LC, LN, 4), "d_point_counts null");
  REFUSED(raw(PTS, PC, 0, LN, 4), "d_line_counts null");
  REFUSED(raw(PTS, PC, LC, 0, 4), "d_lines null with line_capacity > 0");
  REFUSED(raw(PTS + 4, PC, LC, LN, 4), "d_points 4-byte aligned only");
  for (unsigned o = 1; o < 4; ++o) {
    REFUSED(raw(PTS, PC + o, LC, LN, 4), "d_point_counts + %u", o);
    REFUSED(raw(PTS, PC, LC + o, LN, 4), "d_line_counts + %u", o);
    REFUSED(raw(PTS, PC, LC, LN + o, 4), "d_lines + %u", o);
  }
  for (int n : { 0, -1, 5, 1 << 30 }) REFUSED(raw(PTS, PC, LC, LN, 4, 100, n), "nframes %d of 4", n);
  VCHECK(!raw(PTS, PC, LC, LN, 4, 100, 4).error, "nframes = max");
  for (double v : { 0.0, -1.0, INF, -INF, NaN }) {
    REFUSED(plan(64, 48, 1, v, DEG), "rho %g", v);
    REFUSED(plan(64, 48, 1, 1, v), "theta %g", v);
  }
  for (double v : { INF, -INF, NaN }) {
    REFUSED(plan(64, 48, 1, 1, DEG, HOUGH_SCRATCH_BYTES, 16, 1000, 1024, 10, v, PI), "min_theta %g", v);
    REFUSED(plan(64, 48, 1, 1, DEG, HOUGH_SCRATCH_BYTES, 16, 1000, 1024, 10, 0, v), "max_theta %g", v);
  }
  REFUSED(plan(64, 48, 1, 1, DEG, HOUGH_SCRATCH_BYTES, 16, 1000, 1024, 10, 1.0, 0.5), "max_theta < min_theta");
  VCHECK(!plan(64, 48, 1, 1, DEG, HOUGH_SCRATCH_BYTES, 16, 1000, 1024, 10, 1.0, 1.0).error, "max_theta == min_theta: one angle");
  REFUSED(plan(64, 48, 1, 1, DEG, HOUGH_SCRATCH_BYTES, 16, 1000, 1024, -1), "threshold -1");
  VCHECK(!plan(64, 48, 1, 1, DEG, HOUGH_SCRATCH_BYTES, 16, 1000, 1024, 0).error && !plan(64, 48, 1, 1, DEG, HOUGH_SCRATCH_BYTES, 16, 1000, 1024, 0x7FFFFFFF).error, "thresholds 0 and INT_MAX");
  // an accumulator row and LDS: numrho + 2 = 40960 words fit, 40961 do not.  W + H = 20478: 2 (W + H) + 1 = 40957, rho 1 -> numrho 40957
  {
    const HoughPlan P = plan(20000, 479, 1, 1, PI / 2);  // 2 * 20479 + 1 = 40959 -> 40961 words
    VCHECK(holds_nothing(P), "a row of 40961 words");
    const HoughPlan Q = plan(20000, 478, 1, 1, PI / 2);  // 40957 -> 40959 words
    VCHECK(!Q.error && Q.hp.numrho == 40957 && Q.hp.rows == 1, "a row of 40959 words: %s rows %d", Q.error ? Q.error : "", Q.hp.rows);
    int a = 0, r = 0;
    VCHECK(!hough_geometry(20479, 0 + 1, 40961.0 / 40958.0, PI / 2, 0, PI, &a, &r) && r == 40958, "numrho %d: exactly 160 KiB", r);
    VCHECK(hough_geometry(20479, 1, 40961.0 / 40959.0, PI / 2, 0, PI, &a, &r) != nullptr, "numrho 40959: a word too many");
  }
  REFUSED(plan(64, 48, 1, 1e-6, DEG), "a tiny rho");
  REFUSED(plan(1, 1, 1, 1, 1e-9), "(numangle + 2) * (numrho + 2) >= 2^31");
  REFUSED(plan(1, 1, 1, 1, 1e-300), "numangle beyond any integer");
  REFUSED(plan(64, 48, 1, 1, DEG, HOUGH_SCRATCH_BYTES, 16, 1000, 1024, 10, -1e308, 1e308), "max_theta - min_theta overflows");
  REFUSED(plan(64, 48, 2, 1, DEG, HOUGH_SCRATCH_BYTES, SIZE_MAX / 12 / 2 + 1), "line_capacity * 12 * nframes overflows");
  VCHECK(!plan(64, 48, 2, 1, DEG, HOUGH_SCRATCH_BYTES, SIZE_MAX / 12 / 2).error, "the largest line_capacity");
  REFUSED(plan(64, 48, 2, 1, DEG, HOUGH_SCRATCH_BYTES, 16, SIZE_MAX / 8 / 2 + 1), "point_capacity * 8 * nframes overflows");
  VCHECK(!plan(64, 48, 2, 1, DEG, HOUGH_SCRATCH_BYTES, 16, SIZE_MAX / 8 / 2).error, "the largest point_capacity");
}

static void shapes()
{
  // 1080p at rho 1, theta pi / 180: rows of 6003 words = 24012 bytes: six fit LDS, two leave room for three workgroups per CU
  for (int n : { 1, 2, 8, 9, 43, 58, 59, 64, 200, 1024 }) {
    const HoughPlan P = plan(1920, 1080, n, 1, DEG);
    const size_t accum = (size_t)182 * 6003 * 4, peaks = (size_t)180 * 3001 * 8, items = 180 * 4, per = accum + peaks + items;
    const int fpp = (int)std::min<size_t>((size_t)n, HOUGH_SCRATCH_BYTES / per);
    VCHECK(!P.error && P.hp.numangle == 180 && P.hp.numrho == 6001 && P.frame_accum_bytes == accum && P.frame_peaks_bytes == peaks && P.frame_items_bytes == items && P.hp.peak_cap == (size_t)180 * 3001,
           "1080p n %d: geometry and scratch per frame", n);
    VCHECK(P.frames == n && P.frames_per_pass == fpp && P.passes == (n + fpp - 1) / fpp && P.scratch_bytes == (size_t)fpp * per && P.scratch_bytes <= HOUGH_SCRATCH_BYTES, "1080p n %d: %d per pass, %d passes", n,
           P.frames_per_pass, P.passes);
    int rows = 2;
    while (rows > 1 && (long long)fpp * ((180 + rows - 1) / rows) < HOUGH_CUS) --rows;
    VCHECK(P.hp.rows == rows && P.hp.groups == (180 + rows - 1) / rows && P.total_work == (long long)n * P.hp.groups && P.vote_grid == (unsigned)(fpp * P.hp.groups), "1080p n %d: rows %d groups %d", n, P.hp.rows, P.hp.groups);
    VCHECK((long long)P.hp.rows * 6003 * 4 <= HOUGH_LDS_BYTES && P.hp.nframes == fpp && P.rows_grid == (unsigned)((fpp * 180 + 3) / 4) && P.scan_grid == (unsigned)((fpp + 3) / 4)
           && P.rank_grid_x == (unsigned)((180 * 3001 + 255) / 256) && P.rank_grid_y == (unsigned)fpp, "1080p n %d: grids", n);
  }
  VCHECK(plan(1920, 1080, 1, 1, DEG).hp.rows == 1 && plan(1920, 1080, 2, 1, DEG).hp.rows == 1 && plan(1920, 1080, 3, 1, DEG).hp.rows == 2 && plan(1920, 1080, 9, 1, DEG).hp.rows == 2, "pinned: 1, 1, 2 and 2 rows at 1, 2, 3 and 9 frames of 1080p");
  // the LDS share of a workgroup: (160 KiB / 3) / row bytes rows -- 250x200 at rho 0.3: 3003 + 2 words = 12020 bytes: 4; rho 0.1 at 1080p: one row of 240 KB does not fit at all, rho 0.3: 80 KB, one row
  VCHECK(hough_rows_per_group(32, 3003, 1000) == 4 && hough_max_rows(32, 3003) == 8 && hough_rows_per_group(180, 20003, 1000) == 1 && hough_max_rows(180, 20003) == 2 && hough_rows_per_group(180, 6001, 1000) == 2
         && hough_max_rows(180, 6001) == 6 && hough_rows_per_group(180, 225, 1000) == 8 && hough_rows_per_group(5, 225, 1000) == 5 && hough_rows_per_group(180, 13650, 1000) == 1 && hough_rows_per_group(180, 13651 - 2, 1000) == 1,
         "rows by the LDS share");
  VCHECK(plan(1920, 1080, 1, 1, DEG, HOUGH_SCRATCH_BYTES, 0).rank_grid_x == 0 && plan(1920, 1080, 1, 1, DEG, HOUGH_SCRATCH_BYTES, 0).rank_grid_y == 0, "no ranking at line_capacity 0");
  // small frames: HOUGH_MAX_ROWS bounds the rows once the batch fills the chip
  {
    const HoughPlan P = plan(64, 48, 1024, 1, DEG, HOUGH_SCRATCH_BYTES, 16, 1000, 1024);
    VCHECK(!P.error && P.hp.rows == HOUGH_MAX_ROWS && P.hp.groups == 23 && P.frames_per_pass == 816 && P.passes == 2 && P.total_work == 1024 * 23, "64x48 x 1024: rows %d groups %d", P.hp.rows, P.hp.groups);
    const HoughPlan Q = plan(64, 48, 1, 1, 4.0);
    VCHECK(!Q.error && Q.hp.numangle == 1 && Q.hp.rows == 1 && Q.hp.groups == 1 && Q.total_work == 1, "one angle");
    const HoughPlan Z = plan(1, 1, 1, 1e9, DEG);
    VCHECK(!Z.error && Z.hp.numrho == 0 && Z.hp.peak_cap == 0 && Z.rank_grid_x == 0 && Z.frame_accum_bytes == (size_t)182 * 2 * 4, "numrho 0: no cell can be a peak");
  }
  // a pass holds 65535 frames at most (a frame is a row of k_hough_rank's grid), however small the frames: more passes instead
  {
    const HoughPlan P = plan_hough_lines(1, 1, 200000, PTS, PC, 4, 70000, 1, 4.0, 0, 0, PI, LC, LN, 2, HOUGH_SCRATCH_BYTES);
    VCHECK(!P.error && P.hp.numangle == 1 && P.hp.numrho == 5 && P.frames_per_pass == 65535 && P.passes == 2 && P.rank_grid_y == 65535 && P.hp.nframes == 65535 && P.total_work == 70000, "70000 tiny frames: %d per pass, %d passes",
           P.frames_per_pass, P.passes);
    const HoughParams h = hough_pass(P, 1, 0x70000000u, 0x60000000u);
    VCHECK(h.nframes == 70000 - 65535 && (uintptr_t)h.point_counts == PC + 4 * (size_t)65535, "the second pass: %d frames", h.nframes);
    const HoughPlan Q = plan_hough_lines(1, 1, 200000, PTS, PC, 4, 65535, 1, 4.0, 0, 0, PI, LC, LN, 2, HOUGH_SCRATCH_BYTES);
    VCHECK(!Q.error && Q.frames_per_pass == 65535 && Q.passes == 1, "65535 tiny frames: one pass");
  }
  // forced rows (HC_OPT_TEST_HOUGH_ROWS): taken as given up to what LDS, HOUGH_MAX_ROWS and numangle allow, whatever the batch
  for (int n : { 1, 32 })
    for (int forced = 1; forced <= 10; ++forced) {
      const HoughPlan P = plan_hough_lines(1920, 1080, 1024, PTS, PC, 1000, n, 1, DEG, 10, 0, PI, LC, LN, 16, HOUGH_SCRATCH_BYTES, forced);
      const int rows = std::min(forced, 6);
      VCHECK(!P.error && P.hp.rows == rows && P.hp.groups == (180 + rows - 1) / rows && P.total_work == (long long)n * P.hp.groups, "1080p n %d, %d rows forced: %d", n, forced, P.hp.rows);
      const HoughPlan S = plan_hough_lines(64, 48, 1024, PTS, PC, 1000, n, 1, 4.0, 10, 0, PI, LC, LN, 16, HOUGH_SCRATCH_BYTES, forced);
      VCHECK(!S.error && S.hp.rows == 1 && S.hp.groups == 1, "one angle, %d rows forced", forced);
      const HoughPlan M = plan_hough_lines(64, 48, 1024, PTS, PC, 1000, n, 1, DEG, 10, 0, PI, LC, LN, 16, HOUGH_SCRATCH_BYTES, forced);
      VCHECK(!M.error && M.hp.rows == std::min(forced, HOUGH_MAX_ROWS), "64x48, %d rows forced: %d", forced, M.hp.rows);
    }
  // the scratch bound: one frame, one frame minus a byte, n frames
  {
    const HoughPlan F = plan(64, 48, 5, 1, DEG);
    const size_t per = F.frame_accum_bytes + F.frame_peaks_bytes + F.frame_items_bytes;
    VCHECK(!F.error && per == (size_t)182 * 227 * 4 + (size_t)180 * 113 * 8 + 720 && F.passes == 1 && F.frames_per_pass == 5, "64x48: %zu bytes per frame", per);
    REFUSED(plan(64, 48, 5, 1, DEG, per - 1), "a bound of one frame minus a byte");
    REFUSED(plan(64, 48, 5, 1, DEG, 0), "a bound of nothing");
    for (int k = 1; k <= 6; ++k)
      for (size_t extra : { (size_t)0, per - 1 }) {
        const HoughPlan P = plan(64, 48, 5, 1, DEG, k * per + extra);
        const int fpp = std::min(k, 5);
        VCHECK(!P.error && P.frames_per_pass == fpp && P.passes == (5 + fpp - 1) / fpp && P.scratch_bytes == fpp * per && P.total_work == 5ll * P.hp.groups, "a bound of %d frames + %zu: %d per pass, %d passes", k, extra,
               P.frames_per_pass, P.passes);
        // the passes cover the batch once, on pointers inside the scratch
        const uintptr_t S = 0x70000000u, T = 0x60000000u;
        int seen = 0;
        for (int q = 0; q < P.passes; ++q) {
          const HoughParams h = hough_pass(P, q, S, T);
          VCHECK(h.nframes >= 1 && h.nframes <= fpp && (uintptr_t)h.points == PTS + (size_t)seen * 1000 * 8 && (uintptr_t)h.point_counts == PC + 4 * (size_t)seen && (uintptr_t)h.line_counts == LC + 4 * (size_t)seen
                 && (uintptr_t)h.lines == LN + (size_t)seen * 16 * 12, "pass %d of %d: caller pointers", q, P.passes);
          VCHECK((uintptr_t)h.peaks == S && (uintptr_t)h.accum == S + fpp * P.frame_peaks_bytes && (uintptr_t)h.items == S + fpp * (P.frame_peaks_bytes + P.frame_accum_bytes)
                 && (uintptr_t)h.items + (size_t)fpp * P.frame_items_bytes == S + P.scratch_bytes, "pass %d: scratch pointers", q);
          VCHECK((uintptr_t)h.tab_cos == T && (uintptr_t)h.tab_sin == T + 4 * 180 && (uintptr_t)h.tab_theta == T + 8 * 180 && h.rows == P.hp.rows && h.groups == P.hp.groups, "pass %d: tables", q);
          seen += h.nframes;
        }
        VCHECK(seen == 5, "the passes hold %d of 5 frames", seen);
      }
  }
}

static void table_refusals()
{
  float c[8], s[8], t[8];
  for (float *p : { c, s, t })
    for (int i = 0; i < 8; ++i) p[i] = -77.0f;
  int a = -7, r = -7;
  auto clean = [&]() {
    bool ok = a == -7 && r == -7;
    for (float *p : { c, s, t })
      for (int i = 0; i < 8; ++i) ok = ok && p[i] == -77.0f;
    return ok;
  };
  VCHECK(hough_tables(64, 48, 1, PI / 4, 0, PI, nullptr, &r, c, s, t, 8) && hough_tables(64, 48, 1, PI / 4, 0, PI, &a, nullptr, c, s, t, 8) && clean(), "null geometry pointers");
  VCHECK(hough_tables(64, 48, 1, PI / 4, 0, PI, &a, &r, c, nullptr, t, 8) && hough_tables(64, 48, 1, PI / 4, 0, PI, &a, &r, nullptr, nullptr, t, 8) && clean(), "some tables only");
  VCHECK(hough_tables(64, 48, 1, PI / 4, 0, PI, &a, &r, c, s, t, 3) && clean(), "table_capacity 3 < numangle 4");
  VCHECK(hough_tables(64, 48, 0, PI / 4, 0, PI, &a, &r, c, s, t, 8) && hough_tables(64, 48, 1, NaN, 0, PI, &a, &r, c, s, t, 8) && hough_tables(64, 48, 1, 1, 2, 1, &a, &r, c, s, t, 8) && clean(), "geometry refusals");
  VCHECK(!hough_tables(64, 48, 1, PI / 4, 0, PI, &a, &r, nullptr, nullptr, nullptr, 0) && a == 4 && r == 225 && c[0] == -77.0f, "geometry only");
  VCHECK(!hough_tables(64, 48, 1, PI / 4, 0, PI, &a, &r, c, s, t, 4) && c[0] == 1.0f && s[0] == 0.0f && t[0] == 0.0f && t[1] == (float)(PI / 4) && c[4] == -77.0f && s[4] == -77.0f && t[4] == -77.0f, "four angles, nothing behind them");
}

static int print_tables(char **v)
{
  const int W = std::atoi(v[0]), H = std::atoi(v[1]);
  const double rho = std::strtod(v[2], nullptr), theta = std::strtod(v[3], nullptr), lo = std::strtod(v[4], nullptr), hi = std::strtod(v[5], nullptr);
  int a = 0, r = 0;
  if (const char *e = hough_tables(W, H, rho, theta, lo, hi, &a, &r, nullptr, nullptr, nullptr, 0)) { std::printf("refused: %s\n", e); return 1; }
  std::vector<float> c(a), s(a), t(a);
  if (hough_tables(W, H, rho, theta, lo, hi, &a, &r, c.data(), s.data(), t.data(), (size_t)a)) return 1;
  std::printf("%d %d\n", a, r);
  for (int n = 0; n < a; ++n) {
    uint32_t w[3];
    std::memcpy(&w[0], &c[n], 4); std::memcpy(&w[1], &s[n], 4); std::memcpy(&w[2], &t[n], 4);
    std::printf("%08x %08x %08x\n", w[0], w[1], w[2]);
  }
  return 0;
}

int main(int argc, char **argv)
{
  if (argc == 8 && !std::strcmp(argv[1], "tables")) return print_tables(argv + 2);
  geometry();
  refusals();
  shapes();
  table_refusals();
  if (g_fail) { std::printf("%ld of %ld checks failed\n", g_fail, g_checks); return 1; }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
