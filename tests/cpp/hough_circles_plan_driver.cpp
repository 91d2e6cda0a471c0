// hough_circles_plan_driver.cpp -- plan_hough_circles, circle_pass and hough_circle_geometry of cudacam_amd/csrc/host_plan.h,
// checked without a GPU (tests/test_hough_circles_plan_cpu.py builds this with g++ under ASan + UBSan): every refusal
// hc_hough_circles_device documents, by its message; scratch bytes, passes, the two grids the launch reads and scratch pointers at their boundaries; the
// guards at 2^20 and 2^31; and that a refused plan holds nothing.  Prints "ok <checks>" or the first violations.
//   hough_circles_plan_driver geometry W H dp min_dist min_radius max_radius     (the doubles as C99 hex floats)
// prints "AW AH min_d2", or "refused: <text>".
//   hough_circles_plan_driver plan W H max_frames { nframes point_capacity pitch frame_stride dp min_dist votes_threshold min_radius
//                                                   max_radius centre_capacity circle_capacity scratch_bound }...
// prints, for each group of twelve, "scratch_bytes passes frames_per_pass" or "refused: <text>" (tests/test_device_op_sequences_cpu.py:
// the circles steps of the seeded chains; a scratch_bound of 0 is the context's default, as hc_set_option takes it).
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace hc;

static long g_checks = 0, g_fail = 0;
#define VCHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL "); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const uintptr_t PT = 0x10000000u, PC = 0x20000000u, DX = 0x30000002u, DY = 0x40000006u, CC = 0x50000000u, CI = 0x60000000u;  // (the planes at even, not 4-byte addresses)
static const double INF = std::numeric_limits<double>::infinity(), NaN = std::numeric_limits<double>::quiet_NaN();

struct Call {
  int W = 64, H = 48, max_frames = 4, n = 2;
  uintptr_t points = PT, point_counts = PC, dy = DY, circle_counts = CC, circles = CI;
  size_t pcap = 1000, ccap = 100, centres = 4096, bound = HOUGH_SCRATCH_BYTES;
  View dx{ DX, 130, 130 * 48 + 6 };
  double dp = 1, min_dist = 5;
  int thr = 10, rmin = 3, rmax = 20;
  CirclePlan plan() const { return plan_hough_circles(W, H, max_frames, points, point_counts, pcap, dx, dy, n, dp, min_dist, thr, rmin, rmax, centres, circle_counts, circles, ccap, bound); }
};

static bool holds_nothing(const CirclePlan &P)
{
  const CirclePlan Z;
  return P.error && P.frames == 0 && P.frames_per_pass == 0 && P.passes == 0 && P.scratch_bytes == 0 && P.frame_accum_bytes == 0 && P.frame_peaks_bytes == 0 && !P.emit && std::memcmp(&P.cp, &Z.cp, sizeof P.cp) == 0;
}
// refused, holding nothing, with a message that contains `text`
#define REFUSED(call, text, ...) do { const CirclePlan R_ = (call).plan(); VCHECK(holds_nothing(R_) && std::strstr(R_.error, text), __VA_ARGS__); } while (0)
#define TAKEN(call, ...) do { const CirclePlan R_ = (call).plan(); VCHECK(!R_.error, __VA_ARGS__); } while (0)

static void refusals()
{
  TAKEN(Call(), "the valid call");
  { Call c; c.points = 0; REFUSED(c, "null argument", "d_points null"); }
  { Call c; c.point_counts = 0; REFUSED(c, "null argument", "d_point_counts null"); }
  { Call c; c.dx.p = 0; REFUSED(c, "null argument", "d_dx null"); }
  { Call c; c.dy = 0; REFUSED(c, "null argument", "d_dy null"); }
  { Call c; c.circle_counts = 0; REFUSED(c, "null argument", "d_circle_counts null"); }
  { Call c; c.circles = 0; REFUSED(c, "d_circles is null with circle_capacity > 0", "d_circles null"); }
  { Call c; c.circles = 0; c.ccap = 0; const CirclePlan P = c.plan(); VCHECK(!P.error && !P.emit, "d_circles null with circle_capacity 0"); }
  { Call c; c.ccap = 0; TAKEN(c, "d_circles given with circle_capacity 0"); }
  for (unsigned o = 1; o < 8; ++o) { Call c; c.points += o; REFUSED(c, "d_points must be 8-byte aligned", "d_points + %u", o); }
  for (unsigned o = 1; o < 4; ++o) {
    { Call c; c.point_counts += o; REFUSED(c, "4-byte aligned", "d_point_counts + %u", o); }
    { Call c; c.circle_counts += o; REFUSED(c, "4-byte aligned", "d_circle_counts + %u", o); }
  }
  for (unsigned o = 1; o < 16; ++o) {
    Call c; c.circles += o; REFUSED(c, "d_circles must be 16-byte aligned", "d_circles + %u", o);
    c.ccap = 0; REFUSED(c, "d_circles must be 16-byte aligned", "d_circles + %u with circle_capacity 0", o);
  }
  { Call c; c.dx.p += 1; REFUSED(c, "multiples of the element size", "d_dx odd"); }
  { Call c; c.dy += 1; REFUSED(c, "multiples of the element size", "d_dy odd"); }
  { Call c; c.dx.pitch = 131; c.dx.fs = 131 * 48; REFUSED(c, "multiples of the element size", "pitch odd"); }
  { Call c; c.dx.fs += 1; REFUSED(c, "multiples of the element size", "frame stride odd"); }
  { Call c; c.dx.pitch = 126; REFUSED(c, "pitch smaller than a row", "pitch < 2 * W"); }
  { Call c; c.dx.pitch = 128; c.dx.fs = 128 * 48; TAKEN(c, "tight planes"); }
  { Call c; c.dx.fs = 130 * 48 - 2; REFUSED(c, "frame stride below height * pitch", "frame stride below a frame"); }
  { Call c; c.n = 1; c.dx.fs = 0; TAKEN(c, "one frame: any frame stride"); }
  { Call c; c.n = 1; c.dx.pitch = (((size_t)1 << 32) / 48 + 2) & ~(size_t)1; REFUSED(c, "4 GiB", "height * pitch >= 2^32"); }
  { Call c; c.n = 1; c.dx.pitch = (0xFFFFFFFFull / 48) & ~(size_t)1; TAKEN(c, "height * pitch just below 2^32"); }
  { Call c; c.n = 1; c.dx.pitch = SIZE_MAX - 1; REFUSED(c, "4 GiB", "a pitch that would wrap"); }
  { Call c; c.dx.p = UINTPTR_MAX - 4001; REFUSED(c, "wraps the address space", "d_dx at the end of the address space"); }
  { Call c; c.dy = UINTPTR_MAX - 4001; REFUSED(c, "wraps the address space", "d_dy at the end of the address space"); }
  for (int n : { 0, -1, 5, 1 << 30 }) { Call c; c.n = n; REFUSED(c, "nframes out of range", "nframes %d of 4", n); }
  for (double v : { 0.0, 0.999, -1.0, INF, -INF, NaN }) { Call c; c.dp = v; REFUSED(c, "dp must be finite and at least 1", "dp %g", v); }
  { Call c; c.dp = 1e300; REFUSED(c, "no cell", "dp 1e300: (float)dp is infinite"); }
  for (double v : { -1.0, -1e-300, INF, -INF, NaN }) { Call c; c.min_dist = v; REFUSED(c, "min_dist must be finite and not negative", "min_dist %g", v); }
  { Call c; c.min_dist = 0; const CirclePlan P = c.plan(); VCHECK(!P.error && P.cp.min_d2 == 0, "min_dist 0"); }
  { Call c; c.min_dist = 1e308; const CirclePlan P = c.plan(); VCHECK(!P.error && P.cp.min_d2 == (1ll << 62), "min_dist 1e308: the bound of 2^62"); }
  { Call c; c.thr = -1; REFUSED(c, "votes_threshold must not be negative", "votes_threshold -1"); }
  { Call c; c.thr = 0; TAKEN(c, "votes_threshold 0"); }
  { Call c; c.thr = 0x7FFFFFFF; TAKEN(c, "votes_threshold INT_MAX"); }
  for (int v : { 0, -1, -0x7FFFFFFF - 1 }) { Call c; c.rmin = v; REFUSED(c, "1 <= min_radius <= max_radius", "min_radius %d", v); }
  { Call c; c.rmin = 21; REFUSED(c, "1 <= min_radius <= max_radius", "max_radius < min_radius"); }
  { Call c; c.rmin = 20; TAKEN(c, "max_radius == min_radius"); }
  { Call c; c.rmin = 1; c.rmax = 4094; TAKEN(c, "4096 histogram words"); }
  { Call c; c.rmin = 1; c.rmax = 4095; REFUSED(c, "4096 words", "4097 histogram words"); }
  { Call c; c.rmin = 1; c.rmax = 0x7FFFFFFF; REFUSED(c, "4096 words", "max_radius INT_MAX"); }
  { Call c; c.rmin = (1 << 20) - 70; c.rmax = (1 << 20) - 65; TAKEN(c, "W + max_radius = 2^20 - 1"); }
  { Call c; c.rmin = (1 << 20) - 70; c.rmax = (1 << 20) - 64; REFUSED(c, "below 2^20", "W + max_radius = 2^20"); }
  { Call c; c.W = 32; c.H = 80; c.dx = View{ DX, 64, 64 * 80 }; c.rmin = (1 << 20) - 90; c.rmax = (1 << 20) - 80; REFUSED(c, "below 2^20", "H + max_radius = 2^20"); }
  { Call c; c.rmin = 0x7FFFFFF0; c.rmax = 0x7FFFFFFF; REFUSED(c, "below 2^20", "W + max_radius beyond int"); }
  { Call c; c.centres = 0; REFUSED(c, "centre_capacity must lie in 1 .. 4096", "centre_capacity 0"); }
  { Call c; c.centres = 4097; REFUSED(c, "centre_capacity must lie in 1 .. 4096", "centre_capacity 4097"); }
  { Call c; c.centres = SIZE_MAX; REFUSED(c, "centre_capacity must lie in 1 .. 4096", "centre_capacity SIZE_MAX"); }
  { Call c; c.centres = 1; const CirclePlan P = c.plan(); VCHECK(!P.error && P.cp.centre_capacity == 1 && P.frame_ranked_bytes == 16 && P.frame_items_bytes == 4, "centre_capacity 1"); }
  { Call c; c.pcap = SIZE_MAX / 8 / 2 + 1; REFUSED(c, "point_capacity * 8 * nframes overflows", "point_capacity overflow"); }
  { Call c; c.pcap = SIZE_MAX / 8 / 2; TAKEN(c, "the largest point_capacity"); }
  { Call c; c.pcap = 0; const CirclePlan P = c.plan(); VCHECK(!P.error && P.cp.vote_groups == 1, "point_capacity 0"); }
  { Call c; c.ccap = SIZE_MAX / 16 / 2 + 1; REFUSED(c, "circle_capacity * 16 * nframes overflows", "circle_capacity overflow"); }
  { Call c; c.ccap = SIZE_MAX / 16 / 2; TAKEN(c, "the largest circle_capacity"); }
  // the accumulator at 2^31 cells: 46341^2 > 2^31 > 46339 * 46340 (frames of that size need max_frames 1 and a view below 4 GiB)
  { Call c; c.W = 46339; c.H = 46339; c.n = 1; c.dx = View{ DX, 2 * 46339, 0 }; c.bound = SIZE_MAX; REFUSED(c, "2^31 cells", "46341 x 46341 cells"); }
  { Call c; c.W = 46338; c.H = 46338; c.n = 1; c.dx = View{ DX, 2 * 46338, 0 }; c.bound = SIZE_MAX; const CirclePlan P = c.plan(); VCHECK(!P.error && P.cp.AW == 46338 && P.frame_accum_bytes == (size_t)46340 * 46340 * 4, "46340 x 46340 cells"); }
  { Call c; c.W = 46339; c.H = 46339; c.n = 1; c.dx = View{ DX, 2 * 46339, 0 }; c.bound = SIZE_MAX; c.dp = 2; TAKEN(c, "the same frame at dp 2"); }
}

static size_t per_frame(int AW, int AH, size_t cc) { return 32 * cc + 8 * (size_t)AH * (size_t)((AW + 1) / 2) + 4 * (size_t)(AH + 2) * (size_t)(AW + 2) + 4 * (size_t)AH + 4 * cc + 8; }

static void shapes()
{
  for (int n : { 1, 2, 3, 5, 8, 64 })
    for (size_t cc : { (size_t)1, (size_t)63, (size_t)4096 })
      for (size_t pcap : { (size_t)0, (size_t)1, (size_t)256, (size_t)257, (size_t)65536, (size_t)65537, (size_t)10000000 })
        for (double dp : { 1.0, 1.5, 2.0 }) {
          Call c; c.W = 1920; c.H = 1080; c.max_frames = 64; c.n = n; c.centres = cc; c.pcap = pcap; c.dp = dp; c.dx = View{ DX, 3842, (size_t)3842 * 1080 + 4 }; c.rmin = 10; c.rmax = 100;
          const CirclePlan P = c.plan();
          const int AW = dp == 1.0 ? 1920 : dp == 1.5 ? 1280 : 960, AH = dp == 1.0 ? 1080 : dp == 1.5 ? 720 : 540;  // (1920 * fl(2 / 3) = 1280.00004 rounds to 1280.0f, 1080 * it to 720.0f)
          const size_t pf = per_frame(AW, AH, cc);
          const int fpp = (int)std::min<size_t>((size_t)n, HOUGH_SCRATCH_BYTES / pf);
          VCHECK(!P.error && P.cp.AW == AW && P.cp.AH == AH && P.frames == n && P.frames_per_pass == fpp && P.passes == (n + fpp - 1) / fpp && P.scratch_bytes == (size_t)fpp * pf,
                 "1080p n %d cc %zu dp %g: AW %d AH %d fpp %d passes %d scratch %zu", n, cc, dp, P.cp.AW, P.cp.AH, P.frames_per_pass, P.passes, P.scratch_bytes);
          const unsigned vg = (unsigned)std::min<size_t>(std::max<size_t>((pcap + 255) / 256, 1), 256);
          VCHECK(P.cp.vote_groups == vg && P.cp.rank_groups == (unsigned)((P.cp.peak_cap + 255) / 256) && (size_t)P.cp.rank_groups * 256 >= P.cp.peak_cap && P.emit,
                 "1080p n %d cc %zu pcap %zu: the grids the launch reads %u %u", n, cc, pcap, P.cp.vote_groups, P.cp.rank_groups);
          VCHECK(P.cp.peak_cap == (size_t)AH * (size_t)((AW + 1) / 2) && P.cp.idp == 1.0f / (float)dp && P.cp.dp == (float)dp && P.cp.min_d2 == (long long)std::ceil(25.0 / dp / dp) && P.cp.threshold == 10
                 && P.cp.min_radius == 10 && P.cp.max_radius == 100 && P.cp.centre_capacity == (int)cc && P.cp.W == 1920 && P.cp.H == 1080 && P.cp.nframes == fpp, "1080p dp %g: the parameters", dp);
          VCHECK(!P.cp.accum && !P.cp.row_items && !P.cp.peaks && !P.cp.npeaks && !P.cp.ranked && !P.cp.kept && !P.cp.nkept && !P.cp.items, "the plan holds no scratch pointer");
          const uintptr_t S = 0x70000000u;
          for (int k = 0; k < P.passes; ++k) {
            const CircleParams q = circle_pass(P, k, S);
            const size_t f0 = (size_t)k * fpp, F = (size_t)fpp;
            VCHECK(q.nframes == std::min(fpp, n - (int)f0) && (uintptr_t)q.points == PT + f0 * pcap * 8 && (uintptr_t)q.point_counts == PC + f0 * 4 && (uintptr_t)q.dx == DX + f0 * c.dx.fs
                   && (uintptr_t)q.dy == DY + f0 * c.dx.fs && (uintptr_t)q.circle_counts == CC + f0 * 4 && (uintptr_t)q.circles == CI + f0 * 100 * 16, "pass %d: the caller's pointers", k);
            uintptr_t at = S;
            bool ok = (uintptr_t)q.ranked == at; at += F * 16 * cc;
            ok = ok && (uintptr_t)q.kept == at; at += F * 16 * cc;
            ok = ok && (uintptr_t)q.peaks == at && at % 8 == 0; at += F * 8 * q.peak_cap;
            ok = ok && (uintptr_t)q.accum == at; at += F * 4 * (size_t)(AH + 2) * (size_t)(AW + 2);
            ok = ok && (uintptr_t)q.row_items == at; at += F * 4 * (size_t)AH;
            ok = ok && (uintptr_t)q.items == at; at += F * 4 * cc;
            ok = ok && (uintptr_t)q.npeaks == at; at += F * 4;
            ok = ok && (uintptr_t)q.nkept == at; at += F * 4;
            VCHECK(ok && at == S + P.scratch_bytes, "pass %d: the scratch sections", k);
          }
        }
  // a small bound: one frame, one frame minus a byte, k frames
  Call c; c.n = 4;
  const size_t pf = per_frame(64, 48, 4096);
  { Call d = c; d.bound = pf; const CirclePlan P = d.plan(); VCHECK(!P.error && P.frames_per_pass == 1 && P.passes == 4 && P.scratch_bytes == pf, "a bound of one frame"); }
  { Call d = c; d.bound = pf - 1; REFUSED(d, "scratch bound", "a bound of one frame minus a byte"); }
  { Call d = c; d.bound = 3 * pf + 5; const CirclePlan P = d.plan(); VCHECK(!P.error && P.frames_per_pass == 3 && P.passes == 2 && circle_pass(P, 1, 0x1000).nframes == 1, "a bound of three frames"); }
  { Call d = c; d.bound = 2 * pf; const CirclePlan P = d.plan(); VCHECK(!P.error && P.frames_per_pass == 2 && P.passes == 2 && P.scratch_bytes == 2 * pf, "a bound of two frames"); }
  { Call d = c; d.circles = 0; d.ccap = 0; d.bound = pf; const CirclePlan P = d.plan(); VCHECK(!P.error && circle_pass(P, 3, 0x1000).circles == nullptr, "no circles pointer to move on"); }
}

static void geometry_refusals()
{
  int aw = -7, ah = -7;
  long long d2 = -7;
  auto clean = [&]() { return aw == -7 && ah == -7 && d2 == -7; };
  VCHECK(hough_circle_geometry(64, 48, 1, 0, 1, 2, nullptr, &ah, &d2) && hough_circle_geometry(64, 48, 1, 0, 1, 2, &aw, nullptr, &d2) && hough_circle_geometry(64, 48, 1, 0, 1, 2, &aw, &ah, nullptr) && clean(), "null pointers");
  VCHECK(hough_circle_geometry(0, 48, 1, 0, 1, 2, &aw, &ah, &d2) && hough_circle_geometry(64, 0, 1, 0, 1, 2, &aw, &ah, &d2) && hough_circle_geometry(64, 48, 0.5, 0, 1, 2, &aw, &ah, &d2)
         && hough_circle_geometry(64, 48, NaN, 0, 1, 2, &aw, &ah, &d2) && hough_circle_geometry(64, 48, 1, -1, 1, 2, &aw, &ah, &d2) && hough_circle_geometry(64, 48, 1, 0, 0, 2, &aw, &ah, &d2)
         && hough_circle_geometry(64, 48, 1, 0, 3, 2, &aw, &ah, &d2) && hough_circle_geometry(64, 48, 1, 0, 1, 4095, &aw, &ah, &d2) && hough_circle_geometry(64, 48, 1e39, 0, 1, 2, &aw, &ah, &d2) && clean(),
         "refusals write nothing");
  VCHECK(!hough_circle_geometry(64, 48, 2, 5, 1, 2, &aw, &ah, &d2) && aw == 32 && ah == 24 && d2 == 7, "64 x 48 at dp 2, min_dist 5: 2.5^2 = 6.25 -> 7");
  VCHECK(!hough_circle_geometry((1 << 20) - 2, 1, 1, 0, 1, 1, &aw, &ah, &d2) && aw == (1 << 20) - 2 && ah == 1, "the widest frame");
  VCHECK(!hough_circle_geometry(1, 1, 1e30, 0, 1, 1, &aw, &ah, &d2) && aw == 1 && ah == 1, "one pixel at a huge dp: one cell");
}

static int print_geometry(char **v)
{
  int aw = 0, ah = 0;
  long long d2 = 0;
  if (const char *e = hough_circle_geometry(std::atoi(v[0]), std::atoi(v[1]), std::strtod(v[2], nullptr), std::strtod(v[3], nullptr), std::atoi(v[4]), std::atoi(v[5]), &aw, &ah, &d2)) {
    std::printf("refused: %s\n", e);
    return 1;
  }
  std::printf("%d %d %lld\n", aw, ah, d2);
  return 0;
}

static int print_plans(int count, char **v)
{
  Call c;
  c.W = std::atoi(v[0]); c.H = std::atoi(v[1]); c.max_frames = std::atoi(v[2]);
  for (char **g = v + 3; g + 12 <= v + count; g += 12) {
    c.n = std::atoi(g[0]); c.pcap = std::strtoull(g[1], nullptr, 10); c.dx = View{ DX, (size_t)std::strtoull(g[2], nullptr, 10), (size_t)std::strtoull(g[3], nullptr, 10) };
    c.dp = std::strtod(g[4], nullptr); c.min_dist = std::strtod(g[5], nullptr); c.thr = std::atoi(g[6]); c.rmin = std::atoi(g[7]); c.rmax = std::atoi(g[8]);
    c.centres = std::strtoull(g[9], nullptr, 10); c.ccap = std::strtoull(g[10], nullptr, 10);
    const size_t bound = std::strtoull(g[11], nullptr, 10);
    c.bound = bound ? bound : HOUGH_SCRATCH_BYTES;
    const CirclePlan P = c.plan();
    if (P.error) std::printf("refused: %s\n", P.error);
    else std::printf("%zu %d %d\n", P.scratch_bytes, P.passes, P.frames_per_pass);
  }
  return 0;
}

int main(int argc, char **argv)
{
  if (argc == 8 && !std::strcmp(argv[1], "geometry")) return print_geometry(argv + 2);
  if (argc >= 5 && (argc - 5) % 12 == 0 && !std::strcmp(argv[1], "plan")) return print_plans(argc - 2, argv + 2);
  refusals();
  shapes();
  geometry_refusals();
  if (g_fail) { std::printf("%ld of %ld checks failed\n", g_fail, g_checks); return 1; }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
