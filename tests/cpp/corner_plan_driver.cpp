// corner_plan_driver.cpp -- plan_corner_response, plan_good_features and feat_pass of cudacam_amd/csrc/host_plan.h, checked without
// a GPU (tests/test_corner_plan_cpu.py builds this with g++ under ASan + UBSan): the strip / chunk geometry and the alignment
// classes, every refusal the two entries document, each beside its nearest neighbour that passes, min_d2 at 0, 1, sqrt 2, 1e9 and
// the 2^62 cap, the passes under lowered scratch bounds, and the key / digit helpers the select is built from (canny_params.h)
// against a sorted model of the cut.
// Prints "ok <checks>" or the first violations.
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstring>
#include <limits>

using namespace hc;

static long g_checks = 0, g_fail = 0;
#define VCHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL "); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const size_t BIG = (size_t)256 << 20;
static const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();

static void response_geometry()
{
  const int ws[] = { 1, 2, 3, 4, 5, 247, 248, 249, 496, 497, 1920 }, strips[] = { 1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 8 };
  const int hs[] = { 1, 2, 63, 64, 65, 129, 1080 }, chunks[] = { 1, 1, 1, 1, 2, 3, 17 };
  for (int i = 0; i < 11; ++i)
    for (int j = 0; j < 7; ++j)
      for (int n : { 1, 3 })
        for (int bits = 0; bits < 64; ++bits) {
          const int W = ws[i], H = hs[j];
          // input alignment class from bits 0..2 (2, 4 or 8), output class from bits 3..5 (4, 8 or 16)
          const size_t ia = (bits & 1) ? 2 : (bits & 2) ? 4 : 8, oa = (bits & 8) ? 4 : (bits & 16) ? 8 : 16;
          const size_t ip = round_up(2 * (size_t)W, 8) + 8 + ((bits & 4) ? ia : 0), op = round_up(4 * (size_t)W, 16) + 16 + ((bits & 32) ? oa : 0);
          const View dx{ 0x10000000u + ia, ip, round_up(ip * H, 8) + ia }, out{ 0x60000000u + oa, op, round_up(op * H, 16) + oa };
          const uintptr_t dy = 0x30000000u + ia;
          const CornerPlan P = plan_corner_response(W, H, 4, dx, dy, out, n, 5, CORNER_HARRIS, 0.04);
          VCHECK(!P.error, "%d x %d bits %x: %s", W, H, bits, P.error ? P.error : "");
          if (P.error) continue;
          const CornerParams &c = P.cp;
          const uintptr_t iall = dx.p | dy | dx.pitch | dx.fs, oall = out.p | out.pitch | out.fs;
          const int want_ia = (iall & 7) == 0 ? 8 : (iall & 3) == 0 ? 4 : 2, want_oa = (oall & 15) == 0 ? 16 : (oall & 7) == 0 ? 8 : 4;
          VCHECK(c.nstrips == strips[i] && c.nchunks == chunks[j] && c.total_items == n * strips[i] * chunks[j], "%d x %d: %d strips %d chunks", W, H, c.nstrips, c.nchunks);
          VCHECK(c.in_align == want_ia && c.out_align == want_oa, "%d x %d bits %x: in_align %d out_align %d", W, H, bits, c.in_align, c.out_align);
          VCHECK(c.dx == (const uint8_t *)dx.p && c.dy == (const uint8_t *)dy && c.out == (uint8_t *)out.p && c.pitch == ip && c.frame_stride == dx.fs && c.out_pitch == op
                 && c.out_frame_stride == out.fs && c.W == W && c.H == H && c.nframes == n && c.block_size == 5 && c.method == CORNER_HARRIS && c.k == 0.04f, "%d x %d: the block", W, H);
        }
  const View dx{ 0x10000000u, 3840, 3840 * 1080 }, out{ 0x60000000u, 7680, 7680 * 1080 };
  const CornerPlan P = plan_corner_response(1920, 1080, 64, dx, 0x30000000u, out, 64, 3, CORNER_MIN_EIGEN, NaN);
  VCHECK(!P.error && P.cp.total_items == 64 * 8 * 17 && P.cp.in_align == 8 && P.cp.out_align == 16 && P.cp.k == 0.0f, "pinned 1080p x 64 (harris_k is ignored with MIN_EIGEN)");
}

static void response_refusals()
{
  const int W = 70, H = 32;
  const size_t r16 = 2 * (size_t)W, r32 = 4 * (size_t)W;
  const View dx{ 0x10000000u, r16, r16 * H }, out{ 0x60000000u, r32 + 4, (r32 + 4) * H };
  const uintptr_t dy = 0x30000000u;
  auto plan = [&](const View &x, uintptr_t y, const View &o, int n = 2, int B = 3, int m = CORNER_HARRIS, double k = 0.04, int mf = 4) { return plan_corner_response(W, H, mf, x, y, o, n, B, m, k); };
  auto refused = [](const CornerPlan &P, const char *text) { return P.error && std::strstr(P.error, text) && !P.cp.dx && !P.cp.out && !P.cp.total_items; };
  VCHECK(!plan(dx, dy, out).error && !plan(dx, dy, out, 4, 7, CORNER_MIN_EIGEN).error, "the valid calls");
  VCHECK(refused(plan(View{ 0, r16, r16 * H }, dy, out), "null") && refused(plan(dx, 0, out), "null") && refused(plan(dx, dy, View{ 0, r32, r32 * H }), "null"), "null pointers");
  for (int B : { -3, 0, 1, 2, 4, 6, 8, 9 }) VCHECK(refused(plan(dx, dy, out, 2, B), "block_size"), "block_size %d", B);
  for (int B : { 3, 5, 7 }) VCHECK(!plan(dx, dy, out, 2, B).error, "block_size %d", B);
  for (int m : { -1, 2, 7 }) VCHECK(refused(plan(dx, dy, out, 2, 3, m), "method"), "method %d", m);
  VCHECK(refused(plan(dx, dy, out, 2, 3, CORNER_HARRIS, NaN), "harris_k") && refused(plan(dx, dy, out, 2, 3, CORNER_HARRIS, INF), "harris_k") && refused(plan(dx, dy, out, 2, 3, CORNER_HARRIS, -INF), "harris_k")
         && !plan(dx, dy, out, 2, 3, CORNER_MIN_EIGEN, NaN).error && !plan(dx, dy, out, 2, 3, CORNER_HARRIS, -1e300).error && !plan(dx, dy, out, 2, 3, CORNER_HARRIS, 0.0).error, "harris_k finite with HARRIS only");
  VCHECK(refused(plan(dx, dy, out, 0), "nframes") && refused(plan(dx, dy, out, -1), "nframes") && refused(plan(dx, dy, out, 5), "nframes") && !plan(dx, dy, out, 4).error && !plan(dx, dy, out, 5, 3, 1, 0.04, 5).error, "nframes within 1 .. the bound");
  // misalignment: odd input addresses / pitch / stride; output not a multiple of 4 (2 is not enough)
  VCHECK(refused(plan(View{ dx.p + 1, r16, r16 * H }, dy, out), "multiples") && refused(plan(dx, dy + 1, out), "multiples") && refused(plan(View{ dx.p, r16 + 1, (r16 + 1) * H }, dy, out), "multiples")
         && refused(plan(View{ dx.p, r16, r16 * H + 1 }, dy, out), "multiples") && !plan(View{ dx.p + 2, r16 + 2, (r16 + 2) * H + 2 }, dy + 6, out).error, "input: even, not more");
  VCHECK(refused(plan(dx, dy, View{ out.p + 2, r32, r32 * H }), "multiples of 4") && refused(plan(dx, dy, View{ out.p, r32 + 2, (r32 + 2) * H }), "multiples of 4")
         && refused(plan(dx, dy, View{ out.p, r32, r32 * H + 2 }), "multiples of 4") && !plan(dx, dy, View{ out.p + 4, r32 + 4, (r32 + 4) * H + 4 }).error, "output: multiples of 4");
  VCHECK(refused(plan(View{ dx.p, r16 - 2, r16 * H }, dy, out), "pitch smaller") && refused(plan(dx, dy, View{ out.p, r32 - 4, r32 * H }), "pitch smaller") && !plan(dx, dy, View{ out.p, r32, r32 * H }).error, "pitches below / equal to a row");
  const size_t huge = ((size_t)1 << 32) / H;
  VCHECK(refused(plan(View{ dx.p, huge, huge * H }, 0x500000000000ull, View{ 0x600000000000ull, r32, r32 * H }, 1), "2^32") && refused(plan(dx, dy, View{ 0x600000000000ull, huge, huge * H }, 1), "2^32")
         && !plan(View{ dx.p, huge - 2, (huge - 2) * H }, 0x500000000000ull, View{ 0x600000000000ull, huge - 4, (huge - 4) * H }, 1).error, "height * pitch >= 2^32 on either side");
  VCHECK(refused(plan(View{ dx.p, r16, r16 * H - 2 }, dy, out, 2), "frame stride") && !plan(View{ dx.p, r16, r16 * H - 2 }, dy, out, 1).error
         && refused(plan(dx, dy, View{ out.p, r32, r32 * H - 4 }, 2), "frame stride") && !plan(dx, dy, View{ out.p, r32, r32 * H - 4 }, 1).error, "a frame stride below height * pitch at n = 2, not at n = 1");
  VCHECK(refused(plan(View{ UINTPTR_MAX - 101, r16, r16 * H }, dy, out, 1), "wraps") && refused(plan(dx, UINTPTR_MAX - 101, out, 1), "wraps") && refused(plan(dx, dy, View{ UINTPTR_MAX - 103, r32, r32 * H }, 1), "wraps"), "views that wrap the address space");
  // overlap of the response with either plane: one shared byte on either side; ranges that touch pass
  const size_t in2 = 2 * r16 * H, out2 = 2 * r32 * H;
  const View o{ 0, r32, r32 * H };
  VCHECK(refused(plan(dx, dy, View{ dx.p, r32, r32 * H }), "overlap") && refused(plan(dx, dy, View{ dy, r32, r32 * H }), "overlap"), "in place");
  VCHECK(refused(plan(dx, dy, View{ dx.p + in2 - 4, o.pitch, o.fs }), "overlap") && !plan(dx, dy, View{ dx.p + in2, o.pitch, o.fs }).error, "the response begins on / behind dx's last bytes");
  VCHECK(refused(plan(dx, dy, View{ dy - out2 + 4, o.pitch, o.fs }), "overlap") && !plan(dx, dy, View{ dy - out2, o.pitch, o.fs }).error, "the response ends on / before dy's first byte");
  VCHECK(!plan(dx, dx.p, out).error, "dx and dy may be the same plane");
  const CornerPlan Z = plan_corner_response(0, H, 4, dx, dy, out, 1, 3, 0, 0), Y = plan_corner_response(W, 0, 4, dx, dy, out, 1, 3, 0, 0);
  VCHECK(Z.error && Y.error, "width and height must be positive");
}

static void features_refusals()
{
  const int W = 70, H = 32;
  const size_t r32 = 4 * (size_t)W;
  const View pl{ 0x10000000u, r32, r32 * H };
  const uintptr_t cnt = 0x30000000u, cor = 0x40000000u, qu = 0x50000000u;
  auto plan = [&](const View &v, int n = 2, double q = 0.01, double md = 10, size_t cc = 4096, uintptr_t c = 0x30000000u, uintptr_t xy = 0x40000000u, uintptr_t ql = 0x50000000u, size_t cap = 100, int mf = 4,
                  size_t bound = BIG) { return plan_good_features(W, H, mf, v, n, q, md, cc, c, xy, ql, cap, bound); };
  auto refused = [](const FeatPlan &P, const char *text) { return P.error && std::strstr(P.error, text) && !P.passes && !P.frames && !P.scratch_bytes && !P.fp.plane && !P.fp.counts; };
  VCHECK(!plan(pl).error && !plan(pl, 4, 1.0, 0.0, 1, cnt, 0, 0, 0).error, "the valid calls (counts only: null corners and quality)");
  VCHECK(refused(plan(View{ 0, r32, r32 * H }), "null") && refused(plan(pl, 2, 0.01, 10, 4096, 0), "null"), "null plane / counts");
  VCHECK(refused(plan(pl, 2, 0.01, 10, 4096, cnt, 0, qu, 1), "d_corners is null") && !plan(pl, 2, 0.01, 10, 4096, cnt, 0, qu, 0).error && !plan(pl, 2, 0.01, 10, 4096, cnt, cor, 0, 1).error, "d_corners null with capacity 1 / 0; d_quality may be null");
  VCHECK(refused(plan(View{ pl.p + 2, r32, r32 * H }), "multiples of 4") && refused(plan(View{ pl.p, r32 + 2, (r32 + 2) * H }), "multiples of 4") && refused(plan(View{ pl.p, r32, r32 * H + 2 }), "multiples of 4")
         && !plan(View{ pl.p + 4, r32 + 4, (r32 + 4) * H + 4 }).error, "the plane: multiples of 4");
  VCHECK(refused(plan(pl, 2, 0.01, 10, 4096, cnt + 2), "d_corner_counts") && !plan(pl, 2, 0.01, 10, 4096, cnt + 4).error, "counts 4-byte aligned");
  VCHECK(refused(plan(pl, 2, 0.01, 10, 4096, cnt, cor + 4), "d_corners must be 8") && !plan(pl, 2, 0.01, 10, 4096, cnt, cor + 8).error, "corners 8-byte aligned");
  VCHECK(refused(plan(pl, 2, 0.01, 10, 4096, cnt, cor, qu + 2), "d_quality") && !plan(pl, 2, 0.01, 10, 4096, cnt, cor, qu + 4).error, "quality 4-byte aligned");
  VCHECK(refused(plan(View{ pl.p, r32 - 4, r32 * H }), "pitch smaller"), "pitch below a row");
  const size_t huge = ((size_t)1 << 32) / H;
  VCHECK(refused(plan(View{ pl.p, huge, huge * H }, 1), "2^32") && !plan(View{ pl.p, huge - 4, (huge - 4) * H }, 1).error, "height * pitch >= 2^32");
  VCHECK(refused(plan(View{ pl.p, r32, r32 * H - 4 }, 2), "frame stride") && !plan(View{ pl.p, r32, r32 * H - 4 }, 1).error, "a frame stride below height * pitch at n = 2");
  VCHECK(refused(plan(View{ UINTPTR_MAX - 103, r32, r32 * H }, 1), "wraps"), "a view that wraps the address space");
  for (double q : { 0.0, -0.5, 1.0000001, 2.0, NaN, INF }) VCHECK(refused(plan(pl, 2, q), "quality_level"), "quality_level %g", q);
  VCHECK(!plan(pl, 2, 1.0).error && !plan(pl, 2, 1e-300).error, "quality_level 1 and tiny");
  for (double md : { -1e-9, -1.0, NaN, INF }) VCHECK(refused(plan(pl, 2, 0.01, md), "min_distance"), "min_distance %g", md);
  VCHECK(!plan(pl, 2, 0.01, 0.0).error && !plan(pl, 2, 0.01, 1e300).error, "min_distance 0 and huge");
  VCHECK(refused(plan(pl, 2, 0.01, 10, 0), "candidate_capacity") && refused(plan(pl, 2, 0.01, 10, 4097), "candidate_capacity") && !plan(pl, 2, 0.01, 10, 1).error && !plan(pl, 2, 0.01, 10, 4096).error, "candidate_capacity 1 .. 4096");
  VCHECK(refused(plan(pl, 0), "nframes") && refused(plan(pl, 5), "nframes") && !plan(pl, 4).error && !plan(pl, 5, 0.01, 10, 4096, cnt, cor, qu, 100, 5).error, "nframes within 1 .. the bound");
  VCHECK(refused(plan(pl, 2, 0.01, 10, 4096, cnt, cor, qu, SIZE_MAX / 16 + 1), "overflows") && !plan(pl, 2, 0.01, 10, 4096, cnt, cor, qu, SIZE_MAX / 16).error, "corner_capacity * 8 * nframes");
  const size_t frame = 40 * 4096 + 2048 * 4 + 32 + 8 * 32;
  VCHECK(plan(pl).frame_bytes == frame && refused(plan(pl, 2, 0.01, 10, 4096, cnt, cor, qu, 100, 4, frame - 1), "scratch bound") && !plan(pl, 2, 0.01, 10, 4096, cnt, cor, qu, 100, 4, frame).error, "one frame above / at the scratch bound");
  // the parameter block
  const FeatPlan P = plan(pl, 3, 0.25, 1.5, 64);
  VCHECK(!P.error && P.fp.plane == (const uint8_t *)pl.p && P.fp.pitch == r32 && P.fp.frame_stride == pl.fs && P.fp.W == W && P.fp.H == H && P.fp.nframes == 3 && P.fp.ngroups == 1 && P.fp.quality == 0.25f
         && P.fp.min_d2 == 3 && P.fp.candidate_capacity == 64 && P.fp.corner_capacity == 100 && P.fp.counts == (u32 *)cnt && P.fp.corners == (float *)cor && P.fp.quality_out == (float *)qu && !P.fp.cand && !P.fp.hist, "the block");
  VCHECK(P.frame_bytes == 40 * 64 + 8192 + 32 + 256 && P.passes == 1 && P.frames_per_pass == 3, "the frame's scratch at capacity 64");
}

static void min_distance()
{
  VCHECK(feat_min_d2(0.0) == 0 && feat_min_d2(1.0) == 1 && feat_min_d2(std::sqrt(2.0)) == 3 && feat_min_d2(2.0) == 4 && feat_min_d2(1e9) == 1000000000000000000ll, "min_d2 at 0, 1, sqrt 2, 2, 1e9");
  VCHECK(feat_min_d2(2147483648.0) == (1ll << 62) && feat_min_d2(1e300) == (1ll << 62) && feat_min_d2(2147483647.0) == (long long)(2147483647.0 * 2147483647.0) && feat_min_d2(2147483647.0) < (1ll << 62) && feat_min_d2(0.5) == 1, "the 2^62 cap");
  for (double md : { 0.1, 0.9, 1.0, 1.4142, 1.5, 2.9, 3.0, 3.0001, 17.25, 1000.5 }) {
    const long long v = feat_min_d2(md);
    VCHECK((double)v >= md * md && (v == 0 || (double)(v - 1) < md * md), "min_d2(%g) = %lld is the smallest", md, v);
  }
}

static void passes()
{
  const int W = 33, H = 70, n = 5;
  const size_t cc = 65, list = 16 * cc, cand = 8 * cc, hist = 8192, state = 32, rows = 8 * (size_t)H, frame = 2 * list + cand + hist + state + rows;
  const View pl{ 0x10000004u, 4 * (size_t)W + 4, (4 * (size_t)W + 4) * H + 12 };
  const uintptr_t scratch = 0x70000000u, cnt = 0x30000000u, cor = 0x40000000u, qu = 0x50000000u;
  struct { size_t bound; int fpp, passes; } cases[] = { { BIG, 5, 1 }, { 5 * frame, 5, 1 }, { 5 * frame - 1, 4, 2 }, { 3 * frame, 3, 2 }, { 2 * frame, 2, 3 }, { 2 * frame - 1, 1, 5 }, { frame, 1, 5 } };
  for (const auto &c : cases)
    for (const size_t cap : { (size_t)7, (size_t)0 }) {
      const FeatPlan P = plan_good_features(W, H, n, pl, n, 0.5, 2.0, cc, cnt, cap ? cor : 0, cap ? qu : 0, cap, c.bound);
      VCHECK(!P.error && P.frames == n && P.frames_per_pass == c.fpp && P.passes == c.passes && P.scratch_bytes == c.fpp * frame && P.frame_bytes == frame && P.fp.ngroups == 3, "bound %zu: %d frames per pass, %d passes (%s)", c.bound,
             P.frames_per_pass, P.passes, P.error ? P.error : "");
      if (P.error) continue;
      int seen = 0;
      for (int k = 0; k < P.passes; ++k) {
        const FeatPass T = feat_pass(P, k, scratch);
        const FeatParams &f = T.fp;
        const int f0 = k * c.fpp, nf = std::min(c.fpp, n - f0);
        const uintptr_t ranked = scratch, kept = ranked + c.fpp * list, cd = kept + c.fpp * list, hs = cd + c.fpp * cand, st = hs + c.fpp * hist, rw = st + c.fpp * state;
        VCHECK(f.nframes == nf && f.plane == (const uint8_t *)pl.p + (size_t)f0 * pl.fs && f.counts == (u32 *)cnt + f0 && f.corners == (cap ? (float *)cor + 2 * cap * f0 : nullptr)
               && f.quality_out == (cap ? (float *)qu + cap * f0 : nullptr), "pass %d: the caller's frames %d ..", k, f0);
        VCHECK(f.ranked == (int32_t *)ranked && f.kept == (int32_t *)kept && f.cand == (u32 *)cd && f.hist == (u32 *)hs && f.state == (u32 *)st && f.rows == (u32 *)rw && rw + nf * rows <= scratch + P.scratch_bytes
               && !(ranked & 15) && !(kept & 15) && !(cd & 7), "pass %d: the sections", k);
        VCHECK(T.zero == hs && T.zero_bytes == c.fpp * hist + nf * state && T.zero + T.zero_bytes <= rw, "pass %d: the zeroed range is the histograms and the state words", k);
        seen += nf;
      }
      VCHECK(seen == n, "bound %zu: the passes cover %d of %d frames", c.bound, seen, n);
    }
}

// the helpers of the select: keys order as the values do, and the digits of the three passes rebuild the key; the cut they find
// (from the top digit down, as k_feat_walk does on its histograms) is the sorted list's
static void select_helpers()
{
  const float vals[] = { 0.0f, -0.0f, -1.0f, 1e-45f, 1e-38f, 1.0f, 1.0000001f, 2.0f, 3.4e38f, INFINITY, NAN, -INFINITY };
  const u32 want[] = { 0, 0, 0, 1, 0, 0x3F800000u, 0x3F800001u, 0x40000000u, 0, 0x7F800000u, 0, 0 };
  for (int i = 0; i < 12; ++i) {
    u32 b;
    std::memcpy(&b, &vals[i], 4);
    const u32 k = feat_key(b);
    VCHECK(i == 4 || i == 8 ? k == b : k == want[i], "key of %g = %08x", (double)vals[i], k);
    VCHECK(((feat_digit(k, 0) << 21) | (feat_digit(k, 1) << 10) | feat_digit(k, 2)) == k && feat_prefix(k, 1) == feat_digit(k, 0) && feat_prefix(k, 2) == (k >> 10) && feat_prefix(k, 0) == 0, "digits of %08x", k);
  }
  VCHECK(feat_shift(0) == 21 && feat_shift(1) == 10 && feat_shift(2) == 0 && FEAT_BINS == 2048 && FEAT_PASSES == 3, "11 + 11 + 10 bits");
  u32 seed = 12345;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
  for (int trial = 0; trial < 300; ++trial) {
    const int N = 1 + (int)(rnd() % 400), cap = 1 + (int)(rnd() % 450);
    std::vector<u32> keys(N);
    // few distinct keys that differ inside one digit or across a digit boundary
    const u32 base[] = { 0x3F800000u, 0x3F800001u, 0x3F8003FFu, 0x3F800400u, 0x3F9FFFFFu, 0x3FA00000u, 0x00000001u, 0x7F800000u };
    for (u32 &k : keys) k = base[rnd() % (trial % 8 + 1)];
    std::vector<u32> sorted(keys);
    std::sort(sorted.begin(), sorted.end(), [](u32 a, u32 b) { return a > b; });
    // the walk: per pass the histogram of the keys that agree with T so far
    u32 T = 0, need = (u32)cap;
    bool all = false;
    for (int pass = 0; pass < FEAT_PASSES && !all; ++pass) {
      std::vector<u32> hist(FEAT_BINS, 0);
      for (u32 k : keys)
        if (feat_prefix(k, pass) == feat_prefix(T, pass)) ++hist[feat_digit(k, pass)];
      u32 above = 0;
      int d = FEAT_BINS - 1;
      for (; d >= 0 && above + hist[d] < need; --d) above += hist[d];
      if (d < 0) { all = true; T = 0; need = 0; break; }
      T |= (u32)d << feat_shift(pass);
      need -= above;
    }
    if (N <= cap) VCHECK(all || (N == cap), "trial %d: %d keys within capacity %d", trial, N, cap);
    if (!all) {
      const u32 gt = (u32)std::count_if(keys.begin(), keys.end(), [&](u32 k) { return k > T; }), eq = (u32)std::count(keys.begin(), keys.end(), T);
      VCHECK(sorted[cap - 1] == T && gt + need == (u32)cap && need >= 1 && need <= eq, "trial %d: T %08x need %u (gt %u eq %u) vs sorted[%d] = %08x", trial, T, need, gt, eq, cap - 1, sorted[cap - 1]);
    }
  }
}

int main()
{
  response_geometry();
  response_refusals();
  features_refusals();
  min_distance();
  passes();
  select_helpers();
  if (g_fail) {
    std::printf("%ld of %ld checks failed\n", g_fail, g_checks);
    return 1;
  }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
