// dist_plan_driver.cpp -- plan_distance_transform of cudacam_amd/csrc/host_plan.h, checked without a GPU
// (tests/test_dist_plan_cpu.py builds this with g++ under ASan + UBSan): every refusal hc_distance_transform_device documents, by
// its message; the grids of both kernels at the workgroup and wave boundaries; the LDS row at its limit; views that touch; and that
// a refused plan holds nothing to launch.  Prints "ok <checks>" or the first violations.
//   dist_plan_driver plan W H max_frames { nframes target dist_type map pitch frame_stride dist dist_pitch dist_frame_stride nearest
//                                          nearest_pitch nearest_frame_stride }...
// prints, for each group of twelve, "col_groups row_groups lds_bytes" or "refused: <text>" (tests/test_device_op_sequences_cpu.py:
// the dist steps of the seeded chains).  map, dist and nearest are addresses, so that the plan sees how the views lie to each
// other -- side by side among them; a nearest of 0 is a call without that plane.
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace hc;

static long g_checks = 0, g_fail = 0;
#define VCHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL "); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const uintptr_t MP = 0x10000003u, DS = 0x20000000u, NR = 0x30000004u;  // (the map at an odd address)

struct Call {
  int W = 200, H = 150, max_frames = 4, n = 2, target = HC_DT_TO_NONZERO, type = HC_DT_F32;
  View map{ MP, 203, 203 * 150 + 7 };
  View dist{ DS, 816, 816 * 150 + 12 };
  View nearest{ NR, 804, 804 * 150 };
  DistPlan plan() const { return plan_distance_transform(W, H, max_frames, map, dist, nearest, n, target, type); }
  void tight(int w, int h, int frames)  // tight views of another size, far from each other
  {
    W = w; H = h; n = frames; max_frames = frames;
    map = View{ MP, (size_t)w, (size_t)w * h };
    dist = View{ DS + ((uintptr_t)1 << 36), 4 * (size_t)w, 4 * (size_t)w * h };
    nearest = View{ NR + ((uintptr_t)1 << 40), 4 * (size_t)w, 4 * (size_t)w * h };
  }
};

static bool holds_nothing(const DistPlan &P)
{
  const DistPlan Z;
  return P.error && std::memcmp(&P.dp, &Z.dp, sizeof P.dp) == 0 && P.dp.col_groups == 0 && P.dp.row_groups == 0 && P.dp.lds_bytes == 0 && !P.dp.map && !P.dp.dist;
}
#define REFUSED(call, text, ...) do { const DistPlan R_ = (call).plan(); VCHECK(holds_nothing(R_) && std::strstr(R_.error, text), __VA_ARGS__); } while (0)
#define TAKEN(call, ...) do { const DistPlan R_ = (call).plan(); VCHECK(!R_.error, __VA_ARGS__); } while (0)

static void refusals()
{
  TAKEN(Call(), "the valid call");
  { Call c; c.map.p = 0; REFUSED(c, "null argument", "d_map null"); }
  { Call c; c.dist.p = 0; REFUSED(c, "null argument", "d_dist null"); }
  { Call c; c.nearest = View{ 0, 0, 0 }; const DistPlan P = c.plan(); VCHECK(!P.error && !P.dp.nearest && P.dp.nearest_pitch == 0 && P.dp.nearest_frame_stride == 0, "no nearest plane"); }
  { Call c; c.nearest = View{ 0, 3, 1 }; const DistPlan P = c.plan(); VCHECK(!P.error && !P.dp.nearest && P.dp.nearest_pitch == 0, "no nearest plane: its pitch and stride are not looked at"); }
  for (int v : { -1, 2, 3, 255, 1 << 30 }) {
    { Call c; c.target = v; REFUSED(c, "target must be HC_DT_TO_NONZERO or HC_DT_TO_ZERO", "target %d", v); }
    { Call c; c.type = v; REFUSED(c, "dist_type must be HC_DT_SQUARED_I32 or HC_DT_F32", "dist_type %d", v); }
  }
  for (int t : { 0, 1 })
    for (int d : { 0, 1 }) { Call c; c.target = t; c.type = d; const DistPlan P = c.plan(); VCHECK(!P.error && P.dp.target == t && P.dp.dist_type == d, "target %d type %d", t, d); }
  for (unsigned o = 1; o < 4; ++o) {
    { Call c; c.dist.p += o; REFUSED(c, "d_dist, dist_pitch and dist_frame_stride must be multiples of 4", "d_dist + %u", o); }
    { Call c; c.dist.pitch += o; c.dist.fs = (c.dist.pitch * 150 + 7) & ~(size_t)3; REFUSED(c, "d_dist, dist_pitch and dist_frame_stride must be multiples of 4", "dist_pitch + %u", o); }
    { Call c; c.dist.fs += o; REFUSED(c, "d_dist, dist_pitch and dist_frame_stride must be multiples of 4", "dist_frame_stride + %u", o); }
    { Call c; c.nearest.p += o; REFUSED(c, "d_nearest, nearest_pitch and nearest_frame_stride must be multiples of 4", "d_nearest + %u", o); }
    { Call c; c.nearest.pitch += o; c.nearest.fs = (c.nearest.pitch * 150 + 7) & ~(size_t)3; REFUSED(c, "d_nearest, nearest_pitch and nearest_frame_stride must be multiples of 4", "nearest_pitch + %u", o); }
    { Call c; c.nearest.fs += o; REFUSED(c, "d_nearest, nearest_pitch and nearest_frame_stride must be multiples of 4", "nearest_frame_stride + %u", o); }
  }
  for (unsigned o = 0; o < 4; ++o) { Call c; c.map.p += o; c.map.pitch = 200 + o; c.map.fs = c.map.pitch * 150 + o; TAKEN(c, "any alignment of the map (%u)", o); }
  { Call c; c.map.pitch = 199; REFUSED(c, "pitch smaller than a row", "pitch < W"); }
  { Call c; c.map.pitch = 200; c.map.fs = 200 * 150; TAKEN(c, "tight maps"); }
  { Call c; c.dist.pitch = 796; REFUSED(c, "dist_pitch smaller than a row of 4-byte distances", "dist_pitch < 4 W"); }
  { Call c; c.nearest.pitch = 796; REFUSED(c, "nearest_pitch smaller than a row of int32 indices", "nearest_pitch < 4 W"); }
  { Call c; c.dist.pitch = 800; c.dist.fs = 800 * 150; c.nearest.pitch = 800; c.nearest.fs = 800 * 150; TAKEN(c, "tight planes"); }
  { Call c; c.map.fs = 203 * 150 - 1; REFUSED(c, "frame stride below height * pitch", "map frame stride below a frame"); }
  { Call c; c.dist.fs = 816 * 150 - 4; REFUSED(c, "frame stride below height * pitch", "dist frame stride below a frame"); }
  { Call c; c.nearest.fs = 804 * 150 - 4; REFUSED(c, "frame stride below height * pitch", "nearest frame stride below a frame"); }
  { Call c; c.n = 1; c.map.fs = 0; c.dist.fs = 0; c.nearest.fs = 0; TAKEN(c, "one frame: any frame stride"); }
  for (int n : { 0, -1, 5, 1 << 30 }) { Call c; c.n = n; REFUSED(c, "nframes out of range", "nframes %d of 4", n); }
  { Call c; c.max_frames = 12; c.n = 12; TAKEN(c, "3 * max_batch frames"); c.n = 13; REFUSED(c, "nframes out of range", "one more"); }
  { Call c; c.max_frames = 1 << 20; c.n = 65536; REFUSED(c, "more than 65535 frames", "65536 frames"); }
  // 2^32 row bytes, on every side
  { Call c; c.n = 1; c.map.pitch = ((size_t)1 << 32) / 150 + 1; REFUSED(c, "4 GiB", "H * pitch >= 2^32"); }
  { Call c; c.n = 1; c.map.pitch = 0xFFFFFFFFull / 150; c.dist.p = (uintptr_t)1 << 40; c.nearest.p = (uintptr_t)1 << 41; TAKEN(c, "H * pitch just below 2^32"); }
  { Call c; c.n = 1; c.map.pitch = SIZE_MAX; REFUSED(c, "4 GiB", "a pitch that would wrap"); }
  { Call c; c.n = 1; c.dist.pitch = ((((size_t)1 << 32) / 150) & ~(size_t)3) + 4; REFUSED(c, "4 GiB", "H * dist_pitch >= 2^32"); }
  { Call c; c.n = 1; c.nearest.pitch = ((((size_t)1 << 32) / 150) & ~(size_t)3) + 4; REFUSED(c, "4 GiB", "H * nearest_pitch >= 2^32"); }
  { Call c; c.n = 1; c.dist.pitch = (0xFFFFFFFFull / 150) & ~(size_t)3; c.map.p = ((uintptr_t)1 << 40) + 1; c.nearest.p = (uintptr_t)1 << 41; TAKEN(c, "H * dist_pitch just below 2^32"); }
  { Call c; c.n = 1; c.dist.pitch = SIZE_MAX - 3; REFUSED(c, "4 GiB", "a dist pitch that would wrap"); }
  { Call c; c.map.p = UINTPTR_MAX - 4001; REFUSED(c, "wraps the address space", "d_map at the end of the address space"); }
  { Call c; c.dist.p = (UINTPTR_MAX - 4003) & ~(uintptr_t)3; REFUSED(c, "wraps the address space", "d_dist at the end of the address space"); }
  { Call c; c.nearest.p = (UINTPTR_MAX - 4003) & ~(uintptr_t)3; REFUSED(c, "wraps the address space", "d_nearest at the end of the address space"); }
  { Call c; c.map.fs = SIZE_MAX / 2; c.map.p = SIZE_MAX / 2 + 100; REFUSED(c, "wraps the address space", "a frame stride that wraps"); }
  // the sizes
  { Call c; c.W = 0; REFUSED(c, "width and height must be positive", "W 0"); }
  { Call c; c.H = -3; REFUSED(c, "width and height must be positive", "H -3"); }
  { Call c; c.W = 0x7FFFFFFF; c.H = 1; REFUSED(c, "width * height reaches 2^31 - 1 pixels", "2^31 - 1 pixels in a row"); }
  { Call c; c.W = 46341; c.H = 46341; REFUSED(c, "width * height reaches 2^31 - 1 pixels", "46341^2 pixels"); }
  { Call c; c.W = 65536; c.H = 32768; REFUSED(c, "width * height reaches 2^31 - 1 pixels", "2^31 pixels"); }
  // the squared diagonal: 46341^2 = 2147488281 > 2^31 - 1 > 46340^2 = 2147395600; W * H stays small
  { Call c; c.tight(2, 46342, 1); REFUSED(c, "the squared diagonal (W - 1)^2 + (H - 1)^2 reaches 2^31 - 1", "2 x 46342"); }
  { Call c; c.tight(2, 46341, 1); const DistPlan P = c.plan(); VCHECK(!P.error && P.dp.row_groups == (46341u + DT_ROWS - 1) / DT_ROWS, "2 x 46341: 1 + 46340^2 fits"); }
  // 2^31 - 1 - 46340^2 = 88047, between 296^2 = 87616 and 297^2 = 88209
  { Call c; c.tight(298, 46341, 1); REFUSED(c, "the squared diagonal", "298 x 46341: 297^2 + 46340^2 = 2^31 - 1 + 162"); }
  { Call c; c.tight(297, 46341, 1); TAKEN(c, "297 x 46341: 296^2 + 46340^2 = 2^31 - 1 - 431 fits"); }
  { Call c; c.tight(16384, 43500, 1); REFUSED(c, "the squared diagonal", "16384 x 43500"); }
  { Call c; c.tight(16384, 43000, 1); TAKEN(c, "16384 x 43000"); }
  // the LDS row
  { Call c; c.tight(DT_MAX_W, 2, 2); const DistPlan P = c.plan(); VCHECK(!P.error && P.dp.lds_bytes == 65536 && P.dp.col_groups == 16384u / DT_COL_THREADS, "W = 16384 passes with 64 KiB of LDS"); }
  { Call c; c.tight(DT_MAX_W + 1, 2, 2); REFUSED(c, "width above the 16384 columns of the row k_dt_rows keeps in LDS", "W = 16385"); }
  { Call c; c.tight(40000, 2, 1); REFUSED(c, "width above the 16384 columns", "W = 40000"); }
  // overlap: byte ranges [p, p + (n - 1) fs + (H - 1) pitch + row); every pair, both orders; views that touch pass
  {
    const uintptr_t B = 0x20000000u;
    const size_t map_bytes = 200 * 150 * 2, plane_bytes = 800 * 150 * 2;
    Call c; c.map = View{ B, 200, 200 * 150 }; c.dist = View{ B + map_bytes, 800, 800 * 150 }; c.nearest = View{ B + map_bytes + plane_bytes, 800, 800 * 150 };
    TAKEN(c, "map | dist | nearest, touching");
    { Call d = c; d.dist.p -= 4; REFUSED(d, "the map and the distance plane overlap", "dist begins 4 bytes inside the map"); }
    { Call d = c; d.nearest.p -= 4; REFUSED(d, "the distance plane and the nearest plane overlap", "nearest begins 4 bytes inside dist"); }
    { Call d = c; d.nearest.p = B + map_bytes - 4; d.dist.p = B + (1u << 24); REFUSED(d, "the map and the nearest plane overlap", "nearest begins 4 bytes inside the map"); }
    { Call d = c; d.dist.p = B - plane_bytes; TAKEN(d, "dist ends where the map begins"); d.dist.p += 4; REFUSED(d, "the map and the distance plane overlap", "dist ends 4 bytes inside the map"); }
    { Call d = c; d.nearest.p = B - plane_bytes; TAKEN(d, "nearest ends where the map begins"); d.nearest.p += 4; REFUSED(d, "the map and the nearest plane overlap", "nearest ends 4 bytes inside the map"); }
    { Call d = c; d.nearest.p = d.dist.p - plane_bytes + 4; d.map.p = B + (1u << 24); REFUSED(d, "the distance plane and the nearest plane overlap", "nearest ends 4 bytes inside dist"); }
    { Call d = c; d.dist.p = B; REFUSED(d, "the map and the distance plane overlap", "dist at the map's base"); }
    { Call d = c; d.nearest.p = d.dist.p; REFUSED(d, "the distance plane and the nearest plane overlap", "one plane for both"); }
    // the two outputs as ROIs of one plane, side by side: their byte ranges interleave, but they share no byte
    const uintptr_t Q = B + (1u << 24);
    { Call d = c; d.dist = View{ Q, 1600, 1600 * 150 + 64 }; d.nearest = View{ Q + 800, 1600, 1600 * 150 + 64 }; TAKEN(d, "side by side in one plane, touching"); }
    { Call d = c; d.dist = View{ Q + 800, 1600, 1600 * 150 }; d.nearest = View{ Q, 1600, 1600 * 150 }; TAKEN(d, "side by side, the nearest plane on the left"); }
    { Call d = c; d.dist = View{ Q, 2000, 2000 * 150 }; d.nearest = View{ Q + 1200, 2000, 2000 * 150 }; TAKEN(d, "side by side with a gap, up to the end of the row"); }
    { Call d = c; d.dist = View{ Q, 1600, 1600 * 150 }; d.nearest = View{ Q + 796, 1600, 1600 * 150 }; REFUSED(d, "the distance plane and the nearest plane overlap", "side by side, one word shared per row"); }
    { Call d = c; d.dist = View{ Q, 1600, 1600 * 150 }; d.nearest = View{ Q + 804, 1600, 1600 * 150 }; REFUSED(d, "the distance plane and the nearest plane overlap", "side by side, the right one runs into the next row"); }
    { Call d = c; d.dist = View{ Q, 1600, 1600 * 150 }; d.nearest = View{ Q + 800, 1604, 1604 * 150 }; REFUSED(d, "the distance plane and the nearest plane overlap", "side by side at different pitches"); }
    { Call d = c; d.dist = View{ Q, 1600, 1600 * 150 }; d.nearest = View{ Q + 800, 1600, 1600 * 150 + 4 }; REFUSED(d, "the distance plane and the nearest plane overlap", "side by side at different frame strides"); }
    { Call d = c; d.n = 1; d.dist = View{ Q, 1600, 0 }; d.nearest = View{ Q + 800, 1600, 44 }; TAKEN(d, "one frame side by side: the frame strides are not looked at"); }
    { Call d = c; d.map = View{ Q + 1600, 2400, 2400 * 150 }; d.dist = View{ Q, 2400, 2400 * 150 }; d.nearest = View{ Q + 800, 2400, 2400 * 150 }; REFUSED(d, "the map and the distance plane overlap", "the map beside the planes: the byte-range rule"); }
  }
}

static void geometry()
{
  {
    const DistPlan P = Call().plan();
    const DistParams &d = P.dp;
    VCHECK(d.col_groups == 4 && d.row_groups == 38 && d.lds_bytes == 800, "200 x 150: %u column groups, %u row groups, %u bytes", d.col_groups, d.row_groups, d.lds_bytes);
    VCHECK((uintptr_t)d.map == MP && (uintptr_t)d.dist == DS && (uintptr_t)d.nearest == NR, "pointers");
    VCHECK(d.pitch == 203 && d.frame_stride == 203 * 150 + 7 && d.dist_pitch == 816 && d.dist_frame_stride == 816 * 150 + 12 && d.nearest_pitch == 804 && d.nearest_frame_stride == 804 * 150, "views");
    VCHECK(d.W == 200 && d.H == 150 && d.nframes == 2 && d.target == HC_DT_TO_NONZERO && d.dist_type == HC_DT_F32, "scalars");
  }
  // the wave (k_dt_cols) and row-group (k_dt_rows) boundaries
  static const int WS[][2] = { { 1, 1 }, { 63, 1 }, { 64, 1 }, { 65, 2 }, { 128, 2 }, { 129, 3 }, { 255, 4 }, { 256, 4 }, { 257, 5 }, { 513, 9 }, { 1920, 30 }, { 4100, 65 }, { 16384, 256 } };
  for (const auto &s : WS) {
    Call c; c.tight(s[0], 3, 2);
    const DistPlan P = c.plan();
    VCHECK(!P.error && P.dp.col_groups == (unsigned)s[1] && P.dp.lds_bytes == 4u * (unsigned)s[0], "W = %d: %u column groups", s[0], P.dp.col_groups);
    VCHECK(!P.error && (long long)P.dp.col_groups * DT_COL_THREADS * DT_COLS_PER_LANE >= s[0] && (long long)(P.dp.col_groups - 1) * DT_COL_THREADS * DT_COLS_PER_LANE < s[0], "W = %d: the groups cover the columns", s[0]);
  }
  static const int HS[][2] = { { 1, 1 }, { 2, 1 }, { 3, 1 }, { 4, 1 }, { 5, 2 }, { 7, 2 }, { 8, 2 }, { 9, 3 }, { 1080, 270 }, { 1081, 271 } };
  static_assert(DT_ROWS == 4 && DT_COL_THREADS == 64 && DT_COLS_PER_LANE == 1 && DT_ROW_THREADS == 256, "the tables of this driver are for these constants");
  for (const auto &s : HS) {
    Call c; c.tight(70, s[0], 1);
    const DistPlan P = c.plan();
    VCHECK(!P.error && P.dp.row_groups == (unsigned)s[1], "H = %d: %u row groups", s[0], P.dp.row_groups);
  }
  for (int w = 1; w <= 600; ++w)
    for (int h : { 1, 2, 3, 4, 5, 31, 32, 33 }) {
      Call c; c.tight(w, h, 3);
      const DistPlan P = c.plan();
      VCHECK(!P.error && P.dp.col_groups == (unsigned)(w + 63) / 64 && P.dp.row_groups == (unsigned)(h + 3) / 4 && P.dp.lds_bytes == 4u * (unsigned)w && P.dp.nframes == 3, "%d x %d", w, h);
    }
}

static int print_plans(int count, char **v)
{
  Call c;
  c.W = std::atoi(v[0]); c.H = std::atoi(v[1]); c.max_frames = std::atoi(v[2]);
  auto num = [](const char *t) { return (size_t)std::strtoull(t, nullptr, 10); };
  for (char **g = v + 3; g + 12 <= v + count; g += 12) {
    c.n = std::atoi(g[0]); c.target = std::atoi(g[1]); c.type = std::atoi(g[2]);
    c.map = View{ (uintptr_t)num(g[3]), num(g[4]), num(g[5]) };
    c.dist = View{ (uintptr_t)num(g[6]), num(g[7]), num(g[8]) };
    c.nearest = View{ (uintptr_t)num(g[9]), num(g[10]), num(g[11]) };
    const DistPlan P = c.plan();
    if (P.error) std::printf("refused: %s\n", P.error);
    else std::printf("%u %u %u\n", P.dp.col_groups, P.dp.row_groups, P.dp.lds_bytes);
  }
  return 0;
}

int main(int argc, char **argv)
{
  if (argc >= 5 && (argc - 5) % 12 == 0 && !std::strcmp(argv[1], "plan")) return print_plans(argc - 2, argv + 2);
  refusals();
  geometry();
  if (g_fail) { std::printf("%ld of %ld checks failed\n", g_fail, g_checks); return 1; }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
