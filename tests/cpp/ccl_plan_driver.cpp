// ccl_plan_driver.cpp -- plan_connected_components and ccl_pass of cudacam_amd/csrc/host_plan.h, checked without a GPU
// (tests/test_ccl_plan_cpu.py builds this with g++ under ASan + UBSan): every refusal hc_connected_components_device documents, by
// its message; tiles, grids, passes and scratch bytes under the default bound and small ones; the guards at 2^31 - 1 pixels and
// 2^32 row bytes; and that a refused plan holds nothing.  Prints "ok <checks>" or the first violations.
//   ccl_plan_driver plan W H max_frames { nframes connectivity map pitch frame_stride labels label_pitch label_frame_stride rows
//                                         capacity scratch_bound }...
// prints, for each group of eleven, "scratch_bytes passes frames_per_pass chunk_rows" or "refused: <text>" (tests/
// test_device_op_sequences_cpu.py: the components steps of the seeded chains).  map and labels are addresses, so that the plan
// sees how the two views lie to each other; rows 0 gives null statistics and centroid pointers; a scratch_bound of 0 is the
// context's default, as hc_set_option takes it.
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace hc;

static long g_checks = 0, g_fail = 0;
#define VCHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL "); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const uintptr_t MP = 0x10000003u, LB = 0x20000000u, CN = 0x30000000u, ST = 0x40000004u, CE = 0x50000008u;  // (the map at an odd address)

struct Call {
  int W = 200, H = 150, max_frames = 4, n = 2, conn = 8;
  View map{ MP, 203, 203 * 150 + 7 };
  View labels{ LB, 816, 816 * 150 + 12 };
  uintptr_t counts = CN, stats = ST, cents = CE;
  size_t cap = 100, bound = HOUGH_SCRATCH_BYTES;
  CclPlan plan() const { return plan_connected_components(W, H, max_frames, map, labels, n, conn, counts, stats, cents, cap, bound); }
};

static bool holds_nothing(const CclPlan &P)
{
  const CclPlan Z;
  return P.error && P.frames == 0 && P.frames_per_pass == 0 && P.passes == 0 && P.scratch_bytes == 0 && P.frame_items_bytes == 0 && !P.stats && std::memcmp(&P.cp, &Z.cp, sizeof P.cp) == 0;
}
#define REFUSED(call, text, ...) do { const CclPlan R_ = (call).plan(); VCHECK(holds_nothing(R_) && std::strstr(R_.error, text), __VA_ARGS__); } while (0)
#define TAKEN(call, ...) do { const CclPlan R_ = (call).plan(); VCHECK(!R_.error, __VA_ARGS__); } while (0)

static void refusals()
{
  TAKEN(Call(), "the valid call");
  { Call c; c.map.p = 0; REFUSED(c, "null argument", "d_map null"); }
  { Call c; c.labels.p = 0; REFUSED(c, "null argument", "d_labels null"); }
  { Call c; c.counts = 0; REFUSED(c, "null argument", "d_counts null"); }
  { Call c; c.stats = 0; REFUSED(c, "d_stats or d_centroids is null with capacity > 0", "d_stats null"); }
  { Call c; c.cents = 0; REFUSED(c, "d_stats or d_centroids is null with capacity > 0", "d_centroids null"); }
  { Call c; c.stats = 0; c.cents = 0; c.cap = 0; const CclPlan P = c.plan(); VCHECK(!P.error && !P.stats && P.cp.row_groups == 0, "null rows with capacity 0"); }
  { Call c; c.cap = 0; const CclPlan P = c.plan(); VCHECK(!P.error && !P.stats, "rows given with capacity 0"); }
  for (int v : { 0, 1, 2, 6, 7, 9, -8, 16 }) { Call c; c.conn = v; REFUSED(c, "connectivity must be 4 or 8", "connectivity %d", v); }
  { Call c; c.conn = 4; const CclPlan P = c.plan(); VCHECK(!P.error && P.cp.connectivity == 4, "connectivity 4"); }
  for (unsigned o = 1; o < 4; ++o) {
    { Call c; c.counts += o; REFUSED(c, "d_counts and d_stats must be 4-byte aligned", "d_counts + %u", o); }
    { Call c; c.stats += o; REFUSED(c, "d_counts and d_stats must be 4-byte aligned", "d_stats + %u", o); }
    { Call c; c.labels.p += o; REFUSED(c, "d_labels, label_pitch and label_frame_stride must be multiples of 4", "d_labels + %u", o); }
    { Call c; c.labels.pitch += o; c.labels.fs = (c.labels.pitch * 150 + 7) & ~(size_t)3;
      REFUSED(c, "d_labels, label_pitch and label_frame_stride must be multiples of 4", "label_pitch + %u", o); }
    { Call c; c.labels.fs += o; REFUSED(c, "d_labels, label_pitch and label_frame_stride must be multiples of 4", "label_frame_stride + %u", o); }
  }
  for (unsigned o = 1; o < 8; ++o) { Call c; c.cents += o; REFUSED(c, "d_centroids must be 8-byte aligned", "d_centroids + %u", o); }
  for (unsigned o = 0; o < 4; ++o) { Call c; c.map.p += o; c.map.pitch = 200 + o; c.map.fs = c.map.pitch * 150 + o; TAKEN(c, "any alignment of the map (%u)", o); }
  { Call c; c.map.pitch = 199; REFUSED(c, "pitch smaller than a row", "pitch < W"); }
  { Call c; c.map.pitch = 200; c.map.fs = 200 * 150; TAKEN(c, "tight maps"); }
  { Call c; c.labels.pitch = 796; REFUSED(c, "label_pitch smaller than a row of int32 labels", "label_pitch < 4 W"); }
  { Call c; c.labels.pitch = 800; c.labels.fs = 800 * 150; TAKEN(c, "tight labels"); }
  { Call c; c.map.fs = 203 * 150 - 1; REFUSED(c, "frame stride below height * pitch", "map frame stride below a frame"); }
  { Call c; c.labels.fs = 816 * 150 - 4; REFUSED(c, "frame stride below height * pitch", "label frame stride below a frame"); }
  { Call c; c.n = 1; c.map.fs = 0; c.labels.fs = 0; TAKEN(c, "one frame: any frame stride"); }
  for (int n : { 0, -1, 5, 1 << 30 }) { Call c; c.n = n; REFUSED(c, "nframes out of range", "nframes %d of 4", n); }
  // 2^32 row bytes, on either side
  { Call c; c.n = 1; c.map.pitch = ((size_t)1 << 32) / 150 + 1; REFUSED(c, "4 GiB", "H * pitch >= 2^32"); }
  { Call c; c.n = 1; c.map.pitch = 0xFFFFFFFFull / 150; c.labels.p = (uintptr_t)1 << 40; TAKEN(c, "H * pitch just below 2^32"); }
  { Call c; c.n = 1; c.map.pitch = SIZE_MAX; REFUSED(c, "4 GiB", "a pitch that would wrap"); }
  { Call c; c.n = 1; c.labels.pitch = ((((size_t)1 << 32) / 150) & ~(size_t)3) + 4; REFUSED(c, "4 GiB", "H * label_pitch >= 2^32"); }
  { Call c; c.n = 1; c.labels.pitch = (0xFFFFFFFFull / 150) & ~(size_t)3; c.map.p = ((uintptr_t)1 << 40) + 1; TAKEN(c, "H * label_pitch just below 2^32"); }
  { Call c; c.n = 1; c.labels.pitch = SIZE_MAX - 3; REFUSED(c, "4 GiB", "a label pitch that would wrap"); }
  { Call c; c.map.p = UINTPTR_MAX - 4001; REFUSED(c, "wraps the address space", "d_map at the end of the address space"); }
  { Call c; c.labels.p = (UINTPTR_MAX - 4003) & ~(uintptr_t)3; REFUSED(c, "wraps the address space", "d_labels at the end of the address space"); }
  { Call c; c.map.fs = SIZE_MAX / 2; c.map.p = SIZE_MAX / 2 + 100; REFUSED(c, "wraps the address space", "a frame stride that wraps"); }
  // 2^31 - 1 pixels: refused before anything about the views is looked at (no view of such a frame passes the 2^32 guard)
  { Call c; c.W = 0x7FFFFFFF; c.H = 1; REFUSED(c, "width * height reaches 2^31 - 1 pixels", "2^31 - 1 pixels in a row"); }
  { Call c; c.W = 46341; c.H = 46341; REFUSED(c, "width * height reaches 2^31 - 1 pixels", "46341^2 pixels"); }
  { Call c; c.W = 65536; c.H = 32768; REFUSED(c, "width * height reaches 2^31 - 1 pixels", "2^31 pixels"); }
  { Call c; c.W = 0x7FFFFFFE; c.H = 1; c.n = 1; c.map.pitch = 0x7FFFFFFE; REFUSED(c, "label_pitch smaller", "2^31 - 2 pixels pass the pixel guard"); }
  { Call c; c.W = 0; REFUSED(c, "width and height must be positive", "W 0"); }
  // overlap: byte ranges [p, p + (n - 1) fs + (H - 1) pitch + row)
  {
    Call c; c.map = View{ 0x20000000u, 200, 200 * 150 };
    const size_t map_bytes = 200 * 150 * 2;
    c.labels = View{ 0x20000000u + map_bytes, 800, 800 * 150 }; TAKEN(c, "labels begin where the map ends");
    c.labels.p -= 4; REFUSED(c, "the map and the label plane overlap", "labels begin 4 bytes inside the map");
    c.labels.p = 0x20000000u - 800 * 150 * 2; TAKEN(c, "labels end where the map begins");
    c.labels.p += 4; REFUSED(c, "the map and the label plane overlap", "labels end 4 bytes inside the map");
    c.labels.p = 0x20000000u; REFUSED(c, "the map and the label plane overlap", "the same base");
  }
  { Call c; c.cap = SIZE_MAX / 20 / 2 + 1; REFUSED(c, "capacity * 20 * nframes overflows size_t", "capacity * 20 * 2"); }
  { Call c; c.cap = SIZE_MAX / 20 / 2; TAKEN(c, "capacity * 20 * 2 just fits"); }
  { Call c; c.cap = SIZE_MAX; REFUSED(c, "overflows size_t", "capacity SIZE_MAX"); }
  { Call c; c.bound = 75; REFUSED(c, "exceeds the context's scratch bound", "a bound below one frame's table"); }
}

static void geometry()
{
  {
    const CclPlan P = Call().plan();   // 200 x 150, 2 frames: 8-row chunks
    const CclParams &c = P.cp;
    VCHECK(c.tiles_x == 4 && c.tiles_y == 5 && c.border_items == 4u * 200 + 3u * 150, "tiles of 200 x 150: %d x %d, %u border pixels", c.tiles_x, c.tiles_y, c.border_items);
    VCHECK(c.chunk_rows == 8 && c.nchunks == 19 && c.total_items == 38, "chunks: %d rows, %d per frame, %d items", c.chunk_rows, c.nchunks, c.total_items);
    VCHECK(P.frame_items_bytes == 76 && P.scratch_bytes == 152 && P.passes == 1 && P.frames_per_pass == 2 && P.frames == 2, "one pass under the default bound");
    VCHECK(P.stats && c.row_groups == 1 && c.capacity == 100 && c.nframes == 2, "rows");
    VCHECK((uintptr_t)c.map == MP && (uintptr_t)c.labels == LB && (uintptr_t)c.counts == CN && (uintptr_t)c.stats == ST && (uintptr_t)c.sums == CE && c.items == nullptr, "pointers");
    VCHECK(c.pitch == 203 && c.frame_stride == 203 * 150 + 7 && c.label_pitch == 816 && c.label_frame_stride == 816 * 150 + 12 && c.W == 200 && c.H == 150 && c.connectivity == 8, "views");
  }
  static const int SIZES[][4] = { { 1, 1, 1, 1 }, { 64, 32, 1, 1 }, { 65, 32, 2, 1 }, { 64, 33, 1, 2 }, { 1920, 1080, 30, 34 }, { 130, 67, 3, 3 } };  // W, H, tiles_x, tiles_y
  for (const auto &s : SIZES) {
    Call c; c.W = s[0]; c.H = s[1]; c.n = 1; c.map = View{ MP, (size_t)s[0], 0 }; c.labels = View{ LB + ((uintptr_t)1 << 36), 4 * (size_t)s[0], 0 };
    const CclPlan P = c.plan();
    VCHECK(!P.error && P.cp.tiles_x == s[2] && P.cp.tiles_y == s[3], "%d x %d: %d x %d tiles", s[0], s[1], P.cp.tiles_x, P.cp.tiles_y);
    VCHECK(!P.error && P.cp.border_items == (unsigned)((s[3] - 1) * s[0] + (s[2] - 1) * s[1]), "%d x %d: border pixels", s[0], s[1]);
    VCHECK(!P.error && P.cp.nchunks == (s[1] + P.cp.chunk_rows - 1) / P.cp.chunk_rows && P.cp.chunk_rows >= 1 && P.cp.chunk_rows <= s[1], "%d x %d: chunks", s[0], s[1]);
  }
  // the row groups: ceil(min(capacity, W * H + 1) / 256), at most 1024
  static const size_t CAPS[][2] = { { 1, 1 }, { 256, 1 }, { 257, 2 }, { 30001, 118 }, { (size_t)1 << 40, 118 } };  // capacity, row groups of 200 x 150
  for (const auto &s : CAPS) {
    Call c; c.cap = s[0]; const CclPlan P = c.plan();
    VCHECK(!P.error && P.cp.row_groups == s[1], "capacity %zu: %u row groups", (size_t)s[0], P.cp.row_groups);
  }
  { Call c; c.W = 1920; c.H = 1080; c.n = 1; c.map = View{ MP, 1920, 0 }; c.labels = View{ LB + ((uintptr_t)1 << 36), 7680, 0 }; c.cap = (size_t)1 << 30;
    const CclPlan P = c.plan(); VCHECK(!P.error && P.cp.row_groups == CCL_ROW_GROUPS, "1080p, a huge capacity: %u row groups", P.cp.row_groups); }
}

static void passes()
{
  for (size_t bound : { (size_t)76, (size_t)151, (size_t)152, (size_t)228, (size_t)303, (size_t)304, (size_t)1 << 20 }) {
    Call c; c.max_frames = 4; c.n = 4; c.bound = bound;
    const CclPlan P = c.plan();
    const int fpp = (int)std::min<size_t>(4, bound / 76);
    VCHECK(!P.error && P.frames_per_pass == fpp && P.passes == (4 + fpp - 1) / fpp && P.scratch_bytes == (size_t)fpp * 76, "bound %zu: %d frames per pass, %d passes", bound, P.frames_per_pass, P.passes);
    if (P.error) continue;
    int seen = 0;
    for (int k = 0; k < P.passes; ++k) {
      const CclParams q = ccl_pass(P, k, 0x70000000u);
      const size_t f0 = (size_t)k * fpp;
      VCHECK(q.nframes == std::min(fpp, 4 - (int)f0) && q.total_items == q.nframes * q.nchunks && (size_t)q.total_items * 4 <= P.scratch_bytes, "bound %zu pass %d: frames", bound, k);
      VCHECK((uintptr_t)q.map == MP + f0 * c.map.fs && (uintptr_t)q.labels == LB + f0 * c.labels.fs && (uintptr_t)q.counts == CN + 4 * f0, "bound %zu pass %d: views", bound, k);
      VCHECK((uintptr_t)q.stats == ST + f0 * 100 * 20 && (uintptr_t)q.sums == CE + f0 * 100 * 16 && (uintptr_t)q.items == 0x70000000u, "bound %zu pass %d: rows", bound, k);
      VCHECK(q.chunk_rows == P.cp.chunk_rows && q.nchunks == P.cp.nchunks && q.tiles_x == P.cp.tiles_x && q.border_items == P.cp.border_items, "bound %zu pass %d: geometry", bound, k);
      seen += q.nframes;
    }
    VCHECK(seen == 4, "bound %zu: the passes cover %d of 4 frames", bound, seen);
  }
  { Call c; c.cap = 0; c.stats = 0; c.cents = 0; c.n = 3; c.bound = 76; const CclPlan P = c.plan();
    VCHECK(!P.error && P.passes == 3, "counts only, a pass per frame");
    if (!P.error) { const CclParams q = ccl_pass(P, 2, 0x70000000u); VCHECK(q.stats == nullptr && q.sums == nullptr && q.nframes == 1, "null rows stay null"); } }
}

static int print_plans(int count, char **v)
{
  Call c;
  c.W = std::atoi(v[0]); c.H = std::atoi(v[1]); c.max_frames = std::atoi(v[2]);
  auto num = [](const char *t) { return (size_t)std::strtoull(t, nullptr, 10); };
  for (char **g = v + 3; g + 11 <= v + count; g += 11) {
    c.n = std::atoi(g[0]); c.conn = std::atoi(g[1]);
    c.map = View{ (uintptr_t)num(g[2]), num(g[3]), num(g[4]) };
    c.labels = View{ (uintptr_t)num(g[5]), num(g[6]), num(g[7]) };
    const bool rows = std::atoi(g[8]) != 0;
    c.stats = rows ? ST : 0; c.cents = rows ? CE : 0;
    c.cap = num(g[9]);
    const size_t bound = num(g[10]);
    c.bound = bound ? bound : HOUGH_SCRATCH_BYTES;
    const CclPlan P = c.plan();
    if (P.error) std::printf("refused: %s\n", P.error);
    else std::printf("%zu %d %d %d\n", P.scratch_bytes, P.passes, P.frames_per_pass, P.cp.chunk_rows);
  }
  return 0;
}

int main(int argc, char **argv)
{
  if (argc >= 5 && (argc - 5) % 11 == 0 && !std::strcmp(argv[1], "plan")) return print_plans(argc - 2, argv + 2);
  refusals();
  geometry();
  passes();
  if (g_fail) { std::printf("%ld of %ld checks failed\n", g_fail, g_checks); return 1; }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
