// thin_plan_driver.cpp -- plan_thinning and thin_pass of cudacam_amd/csrc/host_plan.h, checked without a GPU
// (tests/test_thin_plan_cpu.py builds this with g++ under ASan + UBSan): the plane geometry at word, panel and tile boundaries, the
// alignment flags, every refusal hc_thinning_device documents, each beside a neighbour that passes, and the passes under lowered
// scratch bounds: frames per pass, the short last pass, the offsets of pass k.  Also the bit-sliced decision the kernel makes
// (thin_removed, canny_params.h): the kernel's own text, for every 3 x 3 neighbourhood at every bit position, against the rules of
// include/hipcanny.h written out per pixel.
// Prints "ok <checks>" or the first violations.
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstring>

using namespace hc;

static long g_checks = 0, g_fail = 0;
#define VCHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL "); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const size_t BIG = (size_t)256 << 20;

static void geometry()
{
  // words per row, pinned by hand
  const int ws[] = { 1, 31, 32, 33, 2047, 2048, 2049, 8184 }, words[] = { 1, 1, 1, 2, 64, 64, 65, 256 }, panels[] = { 1, 1, 1, 1, 1, 1, 2, 4 };
  for (int i = 0; i < 8; ++i) VCHECK(thin_row_words(ws[i]) == words[i] && thin_panels(ws[i]) == panels[i], "W %d: %d words, %d panels", ws[i], thin_row_words(ws[i]), thin_panels(ws[i]));
  const int heights[] = { 1, 2, 3, 9, THIN_TILE_ROWS - 1, THIN_TILE_ROWS, THIN_TILE_ROWS + 1, 2 * THIN_TILE_ROWS + 1, 1080 };
  for (int i = 0; i < 8; ++i)
    for (int H : heights)
      for (int n : { 1, 2, 5 })
        for (int method : { THIN_ZHANGSUEN, THIN_GUOHALL })
          for (int mi : { 1, 16, 1024 })
            for (int bits = 0; bits < 64; ++bits) {  // one low bit of each of the six alignment inputs
              const int W = ws[i];
              const size_t ip = ((size_t)W + 3) / 4 * 4 + 4 + (bits & 1), op = ((size_t)W + 3) / 4 * 4 + 8 + ((bits >> 1) & 1);
              const size_t ifs = (ip * H + 3) / 4 * 4 + ((bits >> 2) & 1) * 2, ofs = (op * H + 3) / 4 * 4 + ((bits >> 3) & 1) * 3;
              const View in{ 0x10000000u + ((unsigned)(bits >> 4) & 1), ip, ifs }, out{ 0x40000000u + 2 * ((unsigned)(bits >> 5) & 1), op, ofs };
              const uintptr_t status = (bits & 3) ? 0x70000000u : 0;
              const ThinPlan P = plan_thinning(W, H, false, 5, in, out, n, method, mi, status, BIG);
              const int tiles = (H + THIN_TILE_ROWS - 1) / THIN_TILE_ROWS;
              VCHECK(!P.error && P.row_words == words[i] && P.panels == panels[i] && P.tiles == tiles && P.tile_rows == THIN_TILE_ROWS && P.passes == 1 && P.frames == n && P.frames_per_pass == n,
                     "%d x %d n %d: %d words %d panels %d tiles (%s)", W, H, n, P.row_words, P.panels, P.tiles, P.error ? P.error : "");
              if (P.error) continue;
              VCHECK(P.plane_bytes == (size_t)4 * H * words[i] && P.table_bytes == (size_t)4 * (mi + 1) && P.frame_bytes == 2 * P.plane_bytes + P.table_bytes && P.scratch_bytes == n * P.frame_bytes, "%d x %d: bytes", W, H);
              VCHECK((P.pack.in_aligned != 0) == ((bits & 0x15) == 0) && (P.unpack.out_aligned != 0) == ((bits & 0x2A) == 0), "%d x %d bits %x: in_aligned %d out_aligned %d", W, H, bits, P.pack.in_aligned, P.unpack.out_aligned);
              VCHECK(P.pack.map == (const uint8_t *)in.p && P.pack.pitch == ip && P.pack.frame_stride == ifs && P.pack.W == W && P.pack.H == H && P.pack.nframes == n && P.pack.row_words == words[i]
                     && P.pack.segs == (W + 255) / 256 && P.pack.plane_words == (size_t)H * words[i] && !P.pack.plane_a, "%d x %d: the pack block", W, H);
              VCHECK(P.step.H == H && P.step.nframes == n && P.step.row_words == words[i] && P.step.npanels == panels[i] && P.step.ntiles == tiles && P.step.total_items == n * panels[i] * tiles
                     && P.step.table_words == mi + 1 && P.step.method == method && P.step.plane_words == P.pack.plane_words && !P.step.plane_a && !P.step.plane_b && !P.step.removed, "%d x %d: the step block", W, H);
              VCHECK(P.unpack.out == (uint8_t *)out.p && P.unpack.out_pitch == op && P.unpack.out_frame_stride == ofs && P.unpack.W == W && P.unpack.H == H && P.unpack.nframes == n && P.unpack.status == (u32 *)status
                     && P.unpack.table_words == mi + 1 && P.unpack.max_iterations == mi && P.unpack.segs == P.pack.segs && P.unpack.plane_words == P.pack.plane_words, "%d x %d: the unpack block", W, H);
            }
  // pinned by hand: 1080p, 64 maps: 60 words, one panel, 68 tiles of 16 rows
  const View in{ 0x10000000u, 1920, 1920 * 1080 }, out{ 0x50000000u, 1920, 1920 * 1080 };
  const ThinPlan P = plan_thinning(1920, 1080, false, 64, in, out, 64, THIN_GUOHALL, 16, 0, BIG);
  VCHECK(!P.error && P.row_words == 60 && P.panels == 1 && P.tiles == 68 && P.step.total_items == 64 * 68 && P.plane_bytes == 259200 && P.frame_bytes == 2 * 259200 + 68 && P.passes == 1, "pinned 1080p plan");
}

static void refusals()
{
  const int W = 70, H = 32;
  const size_t row = (size_t)W;
  const View in{ 0x10000000u, row, row * H }, out{ 0x20000000u, row + 4, (row + 4) * H };
  auto plan = [&](const View &i, const View &o, int n = 2, int method = THIN_ZHANGSUEN, int mi = 16, uintptr_t status = 0x30000000u, bool pc = false, int mb = 4, size_t bound = BIG) {
    return plan_thinning(W, H, pc, mb, i, o, n, method, mi, status, bound);
  };
  auto refused = [](const ThinPlan &P, const char *text) {
    return P.error && std::strstr(P.error, text) && !P.passes && !P.frames && !P.scratch_bytes && !P.pack.map && !P.unpack.out && !P.unpack.status && !P.step.total_items;
  };
  VCHECK(!plan(in, out).error && !plan(in, out, 4, THIN_GUOHALL).error && !plan(in, out, 1, THIN_GUOHALL, 1, 0).error, "the valid calls");
  VCHECK(refused(plan(View{ 0, row, row * H }, out), "null") && refused(plan(in, View{ 0, row, row * H }), "null"), "null pointers");
  VCHECK(!plan(in, out, 2, THIN_ZHANGSUEN, 16, 0).error, "a null d_status is fine");
  for (int m : { -1, 2, 3, 100 }) VCHECK(refused(plan(in, out, 2, m), "method"), "method %d", m);
  VCHECK(!plan(in, out, 2, 0).error && !plan(in, out, 2, 1).error, "methods 0 and 1");
  for (int mi : { -5, 0, 1025, 1 << 20 }) VCHECK(refused(plan(in, out, 2, 0, mi), "max_iterations"), "max_iterations %d", mi);
  VCHECK(!plan(in, out, 2, 0, 1).error && !plan(in, out, 2, 0, 1024).error && plan(in, out, 2, 0, 1024).table_bytes == 4100, "max_iterations 1 and 1024");
  for (uintptr_t s : { 0x30000001u, 0x30000002u, 0x30000003u }) VCHECK(refused(plan(in, out, 2, 0, 16, s), "d_status"), "d_status %zx", (size_t)s);
  VCHECK(!plan(in, out, 2, 0, 16, 0x30000004u).error, "d_status 4-byte aligned");
  VCHECK(refused(plan(View{ in.p, row - 1, row * H }, out), "pitch smaller") && refused(plan(in, View{ out.p, row - 1, row * H }), "pitch smaller") && !plan(View{ in.p, row, row * H }, View{ out.p, row, row * H }).error, "pitch below / equal to a row");
  // an odd-aligned view passes
  VCHECK(!plan(View{ in.p + 1, row + 3, (row + 3) * H + 5 }, View{ out.p + 3, row + 1, (row + 1) * H + 1 }).error, "odd base, pitch and frame stride");
  const size_t huge = ((size_t)1 << 32) / H;  // H * pitch = 2^32
  VCHECK(refused(plan(View{ in.p, huge, huge * H }, out, 1), "2^32") && refused(plan(in, View{ out.p, huge, huge * H }, 1), "2^32")
         && !plan(View{ in.p, huge - 1, (huge - 1) * H }, View{ 0x100000000000ull, row, row * H }, 1).error, "height * pitch >= 2^32");
  VCHECK(refused(plan(in, out, 0), "nframes") && refused(plan(in, out, -1), "nframes") && refused(plan(in, out, 5), "nframes") && !plan(in, out, 4).error, "nframes within 1 .. max_batch");
  VCHECK(!plan(in, out, 12, 0, 16, 0, true).error && refused(plan(in, out, 13, 0, 16, 0, true), "nframes out of range"), "3 * max_batch maps on a per-channel context");
  VCHECK(refused(plan(View{ in.p, row, row * H - 1 }, out, 2), "frame stride") && !plan(View{ in.p, row, row * H - 1 }, out, 1).error && refused(plan(in, View{ out.p, row + 4, (row + 4) * H - 1 }, 2), "frame stride"),
         "a frame stride below height * pitch at n = 2, not at n = 1");
  VCHECK(refused(plan(View{ UINTPTR_MAX - 100, row, row * H }, out, 1), "wraps") && refused(plan(in, View{ UINTPTR_MAX - 100, row, row * H }, 1), "wraps"), "a view that wraps the address space");
  // overlap: in place, one shared byte on either side; views that touch pass
  const size_t bytes2 = 2 * row * H;  // n = 2 at stride row * H
  VCHECK(refused(plan(in, View{ in.p, row, row * H }), "overlap"), "in place");
  VCHECK(refused(plan(in, View{ in.p + bytes2 - 1, row, row * H }), "overlap") && !plan(in, View{ in.p + bytes2, row, row * H }).error, "the output begins on / behind the map's last byte");
  VCHECK(refused(plan(View{ out.p + 1, row, row * H }, View{ out.p + 2 - bytes2, row, row * H }), "overlap") && !plan(View{ out.p, row, row * H }, View{ out.p - bytes2, row, row * H }).error,
         "the output ends on / before the map's first byte");
  // one frame's scratch: two planes of 32 rows x 3 words and 17 table words
  const size_t frame = 2 * 32 * 3 * 4 + 17 * 4;
  VCHECK(plan(in, out).frame_bytes == frame && refused(plan(in, out, 2, 0, 16, 0, false, 4, frame - 1), "scratch bound") && !plan(in, out, 2, 0, 16, 0, false, 4, frame).error, "one frame above / at the scratch bound");
  const ThinPlan Z = plan_thinning(0, H, false, 4, in, out, 1, 0, 16, 0, BIG), Y = plan_thinning(W, 0, false, 4, in, out, 1, 0, 16, 0, BIG);
  VCHECK(Z.error && Y.error, "width and height must be positive");
}

static void passes()
{
  const int W = 2049, H = 33, n = 5, mi = 7;  // 65 words, 2 panels, 3 tiles
  const size_t plane = (size_t)4 * H * 65, table = 4 * (mi + 1), frame = 2 * plane + table;
  const View in{ 0x10000001u, 2051, 2051 * (size_t)H + 7 }, out{ 0x20000003u, 2049, 2049 * (size_t)H + 1 };
  const uintptr_t scratch = 0x70000000u, status = 0x60000000u;
  struct { size_t bound; int fpp, passes; } cases[] = { { BIG, 5, 1 }, { 5 * frame, 5, 1 }, { 5 * frame - 1, 4, 2 }, { 3 * frame, 3, 2 }, { 3 * frame - 1, 2, 3 }, { 2 * frame, 2, 3 }, { 2 * frame - 1, 1, 5 }, { frame, 1, 5 } };
  for (const auto &c : cases)
    for (const uintptr_t st : { status, (uintptr_t)0 }) {
      const ThinPlan P = plan_thinning(W, H, false, n, in, out, n, THIN_GUOHALL, mi, st, c.bound);
      VCHECK(!P.error && P.frames == n && P.frames_per_pass == c.fpp && P.passes == c.passes && P.scratch_bytes == c.fpp * frame && P.plane_bytes == plane && P.table_bytes == table,
             "bound %zu: %d frames per pass, %d passes (%s)", c.bound, P.frames_per_pass, P.passes, P.error ? P.error : "");
      if (P.error) continue;
      int seen = 0;
      for (int k = 0; k < P.passes; ++k) {
        const ThinPass T = thin_pass(P, k, scratch);
        const int f0 = k * c.fpp, nf = std::min(c.fpp, n - f0);
        const uintptr_t A = scratch, B = scratch + c.fpp * plane, R = scratch + 2 * c.fpp * plane;
        VCHECK(T.pack.nframes == nf && T.pack.map == (const uint8_t *)in.p + (size_t)f0 * in.fs && T.pack.plane_a == (u32 *)A && !T.pack.in_aligned && T.pack.pitch == in.pitch, "pass %d: the pack reads the caller's frames %d ..", k, f0);
        VCHECK(T.step.nframes == nf && T.step.total_items == nf * 2 * 3 && T.step.plane_a == (u32 *)A && T.step.plane_b == (u32 *)B && T.step.removed == (u32 *)R && T.step.table_words == mi + 1, "pass %d: the step block", k);
        VCHECK(T.unpack.nframes == nf && T.unpack.out == (uint8_t *)out.p + (size_t)f0 * out.fs && T.unpack.plane_a == (const u32 *)A && T.unpack.removed == (const u32 *)R
               && T.unpack.status == (st ? (u32 *)st + 2 * f0 : nullptr) && !T.unpack.out_aligned, "pass %d: the unpack writes the caller's frames and status", k);
        VCHECK(T.tables == R && T.tables_bytes == nf * table && R + T.tables_bytes <= scratch + P.scratch_bytes && B + nf * plane <= R, "pass %d: the tables lie inside the scratch", k);
        seen += nf;
      }
      VCHECK(seen == n, "bound %zu: the passes cover %d of %d frames", c.bound, seen, n);
    }
  const ThinPlan R = plan_thinning(W, H, false, n, in, out, n, THIN_GUOHALL, mi, status, frame - 1);
  VCHECK(R.error && std::strstr(R.error, "scratch bound") && !R.passes, "a bound one byte below one frame");
}

// the rules of include/hipcanny.h for one pixel: is P1 removed by sub-iteration s?  p[2] .. p[9]: the neighbours
static int removed_per_pixel(int method, int s, int p1, const int p[10])
{
  const int p2 = p[2], p3 = p[3], p4 = p[4], p5 = p[5], p6 = p[6], p7 = p[7], p8 = p[8], p9 = p[9];
  if (!p1) return 0;
  if (method == THIN_ZHANGSUEN) {
    const int ring[9] = { p2, p3, p4, p5, p6, p7, p8, p9, p2 };
    int B = 0, A = 0;
    for (int i = 0; i < 8; ++i) {
      B += ring[i];
      A += !ring[i] && ring[i + 1];
    }
    bool ok = B >= 2 && B <= 6 && A == 1;
    if (s == 0) ok = ok && p2 * p4 * p6 == 0 && p4 * p6 * p8 == 0;
    else ok = ok && p2 * p4 * p8 == 0 && p2 * p6 * p8 == 0;
    return ok;
  }
  const int C = ((!p2) & (p3 | p4)) + ((!p4) & (p5 | p6)) + ((!p6) & (p7 | p8)) + ((!p8) & (p9 | p2));
  const int N1 = (p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8), N2 = (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9);
  const int N = std::min(N1, N2);
  const int m = s == 0 ? ((p6 | p7 | (!p9)) & p8) : ((p2 | p3 | (!p5)) & p4);
  return C == 1 && N >= 2 && N <= 3 && m == 0;
}

template <int METHOD, int S>
static void logic_of()
{
  // one neighbourhood alone at every bit, then 32 different neighbourhoods side by side in one word (no bit disturbs another)
  for (int nb = 0; nb < 256; ++nb)
    for (int p1 = 0; p1 < 2; ++p1) {
      int p[10];
      for (int i = 2; i < 10; ++i) p[i] = (nb >> (i - 2)) & 1;
      const int want = removed_per_pixel(METHOD, S, p1, p);
      for (int bit = 0; bit < 32; ++bit) {
        auto B = [&](int v) { return (u32)v << bit; };
        const ThinRow N{ B(p[2]), B(p[9]), B(p[3]) }, C{ B(p1), B(p[8]), B(p[4]) }, S_{ B(p[6]), B(p[7]), B(p[5]) };
        const u32 got = thin_removed<METHOD, S>(N, C, S_);
        VCHECK(got == B(want), "method %d s %d neighbourhood %02x p1 %d bit %d", METHOD, S, nb, p1, bit);
      }
    }
  for (int base = 0; base < 512; base += 7) {
    ThinRow N{ 0, 0, 0 }, C{ 0, 0, 0 }, S_{ 0, 0, 0 };
    u32 want = 0;
    for (int bit = 0; bit < 32; ++bit) {
      const int code = (base + 37 * bit) & 511, p1 = code >> 8;
      int p[10];
      for (int i = 2; i < 10; ++i) p[i] = (code >> (i - 2)) & 1;
      N.c |= (u32)p[2] << bit; N.w |= (u32)p[9] << bit; N.e |= (u32)p[3] << bit;
      C.c |= (u32)p1 << bit; C.w |= (u32)p[8] << bit; C.e |= (u32)p[4] << bit;
      S_.c |= (u32)p[6] << bit; S_.w |= (u32)p[7] << bit; S_.e |= (u32)p[5] << bit;
      want |= (u32)removed_per_pixel(METHOD, S, p1, p) << bit;
    }
    const u32 got = thin_removed<METHOD, S>(N, C, S_);
    VCHECK(got == want, "method %d s %d: 32 neighbourhoods from %d", METHOD, S, base);
  }
}

static void logic()
{
  logic_of<THIN_ZHANGSUEN, 0>();
  logic_of<THIN_ZHANGSUEN, 1>();
  logic_of<THIN_GUOHALL, 0>();
  logic_of<THIN_GUOHALL, 1>();
}

int main()
{
  logic();
  geometry();
  refusals();
  passes();
  if (g_fail) {
    std::printf("%ld of %ld checks failed\n", g_fail, g_checks);
    return 1;
  }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
