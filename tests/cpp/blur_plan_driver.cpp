// blur_plan_driver.cpp -- plan_gaussian_blur, view_end, border_index and gaussian_taps_q8 of cudacam_amd/csrc/host_plan.h /
// canny_params.h, checked without a GPU (tests/test_blur_plan_cpu.py builds this with g++ under ASan + UBSan): the item
// counts at strip and chunk boundaries, the alignment flags, every refusal hc_gaussian_blur_device documents but nframes >
// max_batch (check_views' own), overlapping and touching views, the byte range of a view up to the end of the address space and
// past it, and the border map against its definition.
// Prints "ok <checks>" or the first violations.
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstring>

using namespace hc;

static long g_checks = 0, g_fail = 0;
#define VCHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL "); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const uint16_t T3[3] = { 64, 128, 64 }, T5[5] = { 16, 64, 96, 64, 16 }, T7[7] = { 8, 28, 56, 72, 56, 28, 8 };
static const uint16_t *taps_of(int k) { return k == 3 ? T3 : k == 5 ? T5 : T7; }

static void counts_and_flags()
{
  const int widths[] = { 1, 3, 4, 5, BLUR_STRIP_W - 1, BLUR_STRIP_W, BLUR_STRIP_W + 1, 2 * BLUR_STRIP_W, 2 * BLUR_STRIP_W + 1, 1920 };
  const int heights[] = { 1, 2, 7, BLUR_CHUNK_ROWS - 1, BLUR_CHUNK_ROWS, BLUR_CHUNK_ROWS + 1, 2 * BLUR_CHUNK_ROWS, 2 * BLUR_CHUNK_ROWS + 1, 1080 };
  for (int W : widths)
    for (int H : heights)
      for (int C : { 1, 3 })
        for (int n : { 1, 2, 5 })
          for (int k : { 3, 5, 7 })
            for (int bits = 0; bits < 64; ++bits) {  // one low bit of each of the six alignment inputs
              const size_t row = (size_t)W * C, ip = (row + 3) / 4 * 4 + 4 + (bits & 1), op = (row + 3) / 4 * 4 + 8 + ((bits >> 1) & 1);
              const size_t ifs = (ip * H + 3) / 4 * 4 + ((bits >> 2) & 1) * 2, ofs = (op * H + 3) / 4 * 4 + ((bits >> 3) & 1) * 3;
              const View in{ 0x10000000u + ((unsigned)(bits >> 4) & 1), ip, ifs }, out{ 0x40000000u + 2 * ((unsigned)(bits >> 5) & 1), op, ofs };
              const int border = bits & 1;
              const BlurPlan P = plan_gaussian_blur(W, H, C, in, out, n, k, taps_of(k), border);
              const BlurParams &b = P.bp;
              const int strips = (W + BLUR_STRIP_W - 1) / BLUR_STRIP_W, chunks = (H + BLUR_CHUNK_ROWS - 1) / BLUR_CHUNK_ROWS;
              VCHECK(!P.error && b.nstrips == strips && b.nchunks == chunks && b.total_items == n * strips * chunks, "%d x %d x %d n %d: %d strips, %d chunks, %d items (%s)", W, H, C, n, b.nstrips,
                     b.nchunks, b.total_items, P.error ? P.error : "");
              VCHECK((b.in_aligned != 0) == ((bits & 0x15) == 0) && (b.out_aligned != 0) == ((bits & 0x2A) == 0), "%d x %d x %d bits %x: in_aligned %d out_aligned %d", W, H, C, bits, b.in_aligned, b.out_aligned);
              VCHECK(b.in == (const uint8_t *)in.p && b.in_pitch == ip && b.in_frame_stride == ifs && b.out == (uint8_t *)out.p && b.out_pitch == op && b.out_frame_stride == ofs && b.W == W && b.H == H
                     && b.nframes == n && b.channels == C && b.ksize == k && b.border == border, "%d x %d x %d n %d: views", W, H, C, n);
              bool taps_ok = true;
              for (int i = 0; i <= BLUR_MAX_TAPS; ++i) taps_ok = taps_ok && b.taps[i] == (i < k ? taps_of(k)[i] : 0);
              VCHECK(taps_ok, "%d x %d ksize %d: taps by value, zero behind them", W, H, k);
            }
  // pinned by hand: 1080p, 512 frames: 8 strips x 17 chunks
  const View in{ 0x10000000u, 1920, 1920 * 1080 }, out{ 0x50000000u, 1920, 1920 * 1080 };
  const BlurPlan P = plan_gaussian_blur(1920, 1080, 1, in, out, 512, 5, T5, BLUR_REFLECT_101);
  VCHECK(!P.error && P.bp.nstrips == 8 && P.bp.nchunks == 17 && P.bp.total_items == 512 * 8 * 17 && P.bp.in_aligned && P.bp.out_aligned, "pinned 1080p plan");
}

static void refusals()
{
  const int W = 64, H = 32, C = 3;
  const size_t row = (size_t)W * C;
  const View in{ 0x10000000u, row, row * H }, out{ 0x20000000u, row + 4, (row + 4) * H };
  auto plan = [&](const View &i, const View &o, int n, int k, const uint16_t *t, int border) { return plan_gaussian_blur(W, H, C, i, o, n, k, t, border); };
  VCHECK(!plan(in, out, 2, 3, T3, 0).error && !plan(in, out, 1, 7, T7, 1).error, "the valid calls");
  VCHECK(plan(View{ 0, row, row * H }, out, 1, 3, T3, 0).error && plan(in, View{ 0, row, row * H }, 1, 3, T3, 0).error && plan(in, out, 1, 3, nullptr, 0).error, "null pointers");
  for (int k : { -1, 0, 1, 2, 4, 6, 8, 9 }) VCHECK(plan(in, out, 1, k, T7, 0).error, "ksize %d", k);
  for (int b : { -1, 2, 3, 4 }) VCHECK(plan(in, out, 1, 3, T3, b).error, "border %d", b);
  const uint16_t over[3] = { 257, 0, 0 }, over2[3] = { 0, 65535, 257 }, s255[3] = { 64, 127, 64 }, s257[3] = { 64, 129, 64 }, zero[3] = { 0, 0, 0 }, s255_5[5] = { 16, 64, 95, 64, 16 }, s257_7[7] = { 8, 28, 56, 73, 56, 28, 8 };
  const uint16_t one[3] = { 256, 0, 0 }, last[3] = { 0, 0, 256 }, asym[3] = { 1, 200, 55 };
  VCHECK(plan(in, out, 1, 3, over, 0).error && plan(in, out, 1, 3, over2, 0).error, "a tap above 256");
  VCHECK(plan(in, out, 1, 3, s255, 0).error && plan(in, out, 1, 3, s257, 0).error && plan(in, out, 1, 3, zero, 0).error && plan(in, out, 1, 5, s255_5, 0).error && plan(in, out, 1, 7, s257_7, 0).error, "tap sums of 255, 257, 0");
  VCHECK(!plan(in, out, 1, 3, one, 0).error && !plan(in, out, 1, 3, last, 0).error && !plan(in, out, 1, 3, asym, 0).error, "one-tap and asymmetric sets pass");
  VCHECK(plan(View{ in.p, row - 1, row * H }, out, 1, 3, T3, 0).error && plan(in, View{ out.p, row - 1, row * H }, 1, 3, T3, 0).error, "pitches smaller than a row");
  VCHECK(plan(in, out, 0, 3, T3, 0).error && plan(in, out, -1, 3, T3, 0).error, "nframes below 1");
  VCHECK(plan(View{ in.p, row, row * H - 1 }, out, 2, 3, T3, 0).error && plan(in, View{ out.p, row + 4, (row + 4) * H - 1 }, 2, 3, T3, 0).error && !plan(View{ in.p, row, row * H - 1 }, out, 1, 3, T3, 0).error,
         "frame stride below height * pitch at n = 2, ignored at n = 1");
  const size_t G4 = (size_t)1 << 32;
  VCHECK(plan(View{ in.p, G4 / H, G4 }, out, 1, 3, T3, 0).error && plan(in, View{ out.p, G4 / H, G4 }, 1, 3, T3, 0).error && plan(View{ in.p, (size_t)1 << 31, (size_t)1 << 36 }, out, 1, 3, T3, 0).error, "height * pitch >= 2^32");
  VCHECK(!plan(View{ in.p, G4 / H - 1, G4 }, View{ 0x4000000000ull, row, row * H }, 1, 3, T3, 0).error, "height * pitch just below 2^32");
  VCHECK(plan(in, View{ UINTPTR_MAX - 100, row, row * H }, 1, 3, T3, 0).error && plan(View{ in.p, row, SIZE_MAX / 2 }, out, 3, 3, T3, 0).error, "views that wrap the address space");
  // overlap: the byte ranges [p, p + (n - 1) fs + (H - 1) pitch + C W)
  const size_t ext1 = (size_t)(H - 1) * row + row, ext2 = row * H + ext1;
  VCHECK(plan(in, View{ in.p, row, row * H }, 1, 3, T3, 0).error, "in place");
  VCHECK(plan(in, View{ in.p + ext1 - 1, row, row * H }, 1, 3, T3, 0).error && plan(in, View{ in.p - ext1 + 1, row, row * H }, 1, 3, T3, 0).error, "one shared byte, either side");
  VCHECK(!plan(in, View{ in.p + ext1, row, row * H }, 1, 3, T3, 0).error && !plan(in, View{ in.p - ext1, row, row * H }, 1, 3, T3, 0).error, "touching neighbours, either side");
  VCHECK(plan(in, View{ in.p + ext2 - 1, row, row * H }, 2, 3, T3, 0).error && !plan(in, View{ in.p + ext2, row, row * H }, 2, 3, T3, 0).error && !plan(in, View{ in.p + ext1, row, row * H }, 1, 3, T3, 0).error,
         "batches of 2: the last frame's extent counts");
  VCHECK(plan(View{ in.p, 4 * row, 4 * row * H }, View{ in.p + row, 4 * row, 4 * row * H }, 1, 3, T3, 0).error, "interleaved ROIs of one parent overlap as byte ranges");
  const BlurPlan R = plan(in, View{ in.p, row, row * H }, 1, 3, T3, 0);
  VCHECK(R.error && std::strstr(R.error, "overlap") && R.bp.total_items == 0 && R.bp.in == nullptr, "a refused plan holds nothing to launch");
  VCHECK(plan_gaussian_blur(8184, 1 << 19, 1, View{ 0x10000000u, 8184, (size_t)8184 << 19 }, View{ 0x100000000000ull, 8184, (size_t)8184 << 19 }, 1 << 20, 3, T3, 0).error, "too many work items");
}

// view_end: the byte range [p, p + (n - 1) fs + (H - 1) pitch + row) of a view, and `false` with *end untouched where it wraps
static void view_ends()
{
  const uintptr_t M = UINTPTR_MAX, KEEP = 0x5A5A5A5Au;
  auto ends = [&](const View &v, size_t row, int H, int n, uintptr_t want) { uintptr_t e = KEEP; return view_end(v, row, H, n, &e) && e == want; };
  auto wraps = [&](const View &v, size_t row, int H, int n) { uintptr_t e = KEEP; return !view_end(v, row, H, n, &e) && e == KEEP; };
  for (int H : { 1, 2, 33, 1080 })
    for (int n : { 1, 2, 7 })
      for (size_t row : { (size_t)1, (size_t)192, (size_t)5760 }) {
        const uintptr_t p = 0x10000000u + 3;
        VCHECK(ends(View{ p, row, row * H }, row, H, n, p + (size_t)n * H * row), "tight view %d x %zu x %d ends at p + n H row", H, row, n);
        const size_t pitch = row + 61, fs = pitch * H + 1000;
        VCHECK(ends(View{ p, pitch, fs }, row, H, n, p + (size_t)(n - 1) * fs + (size_t)(H - 1) * pitch + row), "padded, offset view %d x %zu x %d", H, row, n);
        VCHECK(ends(View{ p, pitch, 0 }, row, H, 1, p + (size_t)(H - 1) * pitch + row) && ends(View{ p, pitch, M }, row, H, 1, p + (size_t)(H - 1) * pitch + row), "n = 1 ignores fs (%d x %zu)", H, row);
        VCHECK(ends(View{ p, n > 1 ? 0 : pitch, fs }, row, 1, n, p + (size_t)(n - 1) * fs + row) && (n > 1 || ends(View{ p, M, fs }, row, 1, 1, p + row)), "H = 1 ignores the pitch (%zu x %d)", row, n);
        // the largest view that does not wrap ends at UINTPTR_MAX; one byte more on p, on the pitch, on fs wraps
        const size_t ext = (size_t)(n - 1) * fs + (size_t)(H - 1) * pitch + row;
        const View top{ M - ext, pitch, fs };
        VCHECK(ends(top, row, H, n, M), "the largest view %d x %zu x %d ends at UINTPTR_MAX", H, row, n);
        VCHECK(wraps(View{ top.p + 1, pitch, fs }, row, H, n), "one byte more on p (%d x %zu x %d)", H, row, n);
        // (a pitch one byte larger lengthens the range by H - 1 bytes: moved down by as many, the view fits again)
        if (H > 1) VCHECK(wraps(View{ top.p, pitch + 1, fs }, row, H, n) && ends(View{ top.p - (size_t)(H - 1), pitch + 1, fs }, row, H, n, M), "one byte more on the pitch (%d x %zu x %d)", H, row, n);
        if (n > 1) VCHECK(wraps(View{ top.p, pitch, fs + 1 }, row, H, n) && ends(View{ top.p - (size_t)(n - 1), pitch, fs + 1 }, row, H, n, M), "one byte more on fs (%d x %zu x %d)", H, row, n);
      }
  // at address 0 the whole space is one view: the largest pitch and the largest frame stride by division, one more wraps
  for (int H : { 2, 3, 33, 1080 }) {
    const size_t row = 7, pitch = (M - row) / (size_t)(H - 1);
    VCHECK(ends(View{ 0, pitch, 0 }, row, H, 1, (size_t)(H - 1) * pitch + row) && wraps(View{ 0, pitch + 1, 0 }, row, H, 1), "the largest pitch of %d rows", H);
    VCHECK(ends(View{ M - row - (size_t)(H - 1) * pitch, pitch, 0 }, row, H, 1, M) && wraps(View{ M - row - (size_t)(H - 1) * pitch + 1, pitch, 0 }, row, H, 1), "the largest pitch of %d rows, up to UINTPTR_MAX", H);
  }
  for (int n : { 2, 3, 7, 512 }) {
    const size_t row = 64, pitch = 64, frame = 31 * pitch + row, fs = (M - frame) / (size_t)(n - 1);
    VCHECK(ends(View{ 0, pitch, fs }, row, 32, n, (size_t)(n - 1) * fs + frame) && wraps(View{ 0, pitch, fs + 1 }, row, 32, n), "the largest frame stride of %d frames", n);
    VCHECK(ends(View{ M - frame - (size_t)(n - 1) * fs, pitch, fs }, row, 32, n, M) && wraps(View{ M - frame - (size_t)(n - 1) * fs + 1, pitch, fs }, row, 32, n), "the largest frame stride of %d frames, up to UINTPTR_MAX", n);
  }
  // pitches and strides whose product with H - 1 / n - 1 wraps 64 bits, some of them to a small number
  const size_t HALF = (size_t)1 << 63, THIRD = M / 3 + 1;  // 2 HALF = 0 and 3 THIRD = 2 (mod 2^64)
  VCHECK(wraps(View{ 0x1000, HALF, 0 }, 16, 3, 1) && wraps(View{ 0x1000, THIRD, 0 }, 16, 4, 1) && wraps(View{ 0x1000, M, 0 }, 16, 2, 1) && wraps(View{ 0x1000, M / 2 + 2, 0 }, 16, 3, 1), "pitches whose product with H - 1 wraps");
  VCHECK(wraps(View{ 0x1000, 16, HALF }, 16, 2, 3) && wraps(View{ 0x1000, 16, THIRD }, 16, 2, 4) && wraps(View{ 0x1000, 16, M }, 16, 2, 2) && wraps(View{ 0x1000, 16, SIZE_MAX / 2 }, 16, 2, 3), "frame strides whose product with n - 1 wraps");
  VCHECK(wraps(View{ 0x1000, HALF, HALF }, 16, 3, 3) && wraps(View{ M, 1, 1 }, 1, 1, 1) && ends(View{ M - 1, 1, 1 }, 1, 1, 1, M) && wraps(View{ 0, 16, 0 }, M, 2, 1) && ends(View{ 0, 0, 0 }, M, 1, 1, M), "both at once; the last byte; a row as long as the space");
}

// the overlap cases of refusals(), as (input, output, frames): "view_end of both views, then the interval test" gives the verdict
// plan_gaussian_blur gives
static void overlap_by_view_end()
{
  const int W = 64, H = 32, C = 3;
  const size_t row = (size_t)W * C;
  const View in{ 0x10000000u, row, row * H };
  const size_t ext1 = (size_t)(H - 1) * row + row, ext2 = row * H + ext1;
  const struct { View in, out; int n; bool overlap; } cases[] = {
    { in, View{ in.p, row, row * H }, 1, true }, { in, View{ in.p + ext1 - 1, row, row * H }, 1, true }, { in, View{ in.p - ext1 + 1, row, row * H }, 1, true },
    { in, View{ in.p + ext1, row, row * H }, 1, false }, { in, View{ in.p - ext1, row, row * H }, 1, false }, { in, View{ in.p + ext2 - 1, row, row * H }, 2, true },
    { in, View{ in.p + ext2, row, row * H }, 2, false }, { in, View{ in.p + ext1, row, row * H }, 2, true }, { in, View{ 0x20000000u, row + 4, (row + 4) * H }, 2, false },
    { View{ in.p, 4 * row, 4 * row * H }, View{ in.p + row, 4 * row, 4 * row * H }, 1, true }, { View{ in.p, 4 * row, 4 * row * H }, View{ in.p + row, 4 * row, 4 * row * H }, 2, true },
  };
  for (const auto &c : cases) {
    const BlurPlan P = plan_gaussian_blur(W, H, C, c.in, c.out, c.n, 3, T3, 0);
    uintptr_t e_in = 0, e_out = 0;
    const bool whole = view_end(c.in, row, H, c.n, &e_in) && view_end(c.out, row, H, c.n, &e_out);
    const bool by_ends = c.in.p < e_out && c.out.p < e_in;
    VCHECK(whole && by_ends == c.overlap && (P.error != nullptr) == c.overlap && (!P.error || std::strstr(P.error, "overlap")), "overlap case out %#zx n %d: by view_end %d, plan \"%s\"", (size_t)c.out.p, c.n, (int)by_ends,
           P.error ? P.error : "");
  }
}

static int reflect_by_walking(int i, int n)  // the definition: walk outwards from the axis, turning at the edge pixels without repeating them
{
  if (n == 1) return 0;
  int pos = i < 0 ? 0 : n - 1, dir = i < 0 ? 1 : -1;
  for (int steps = i < 0 ? -i : i - (n - 1); steps > 0; --steps) {
    pos += dir;
    if (pos == 0 || pos == n - 1) dir = -dir;
  }
  return pos;
}

static void borders()
{
  for (int n = 1; n <= 12; ++n)
    for (int i = -30; i <= 41; ++i) {
      const int r = border_index(i, n, BLUR_REFLECT_101), c = border_index(i, n, BLUR_REPLICATE);
      VCHECK(c == (i < 0 ? 0 : i >= n ? n - 1 : i), "replicate %d of %d -> %d", i, n, c);
      VCHECK(r == (i >= 0 && i < n ? i : reflect_by_walking(i, n)), "reflect-101 %d of %d -> %d", i, n, r);
    }
  VCHECK(border_index(-1, 5, 0) == 1 && border_index(-3, 5, 0) == 3 && border_index(5, 5, 0) == 3 && border_index(7, 5, 0) == 1 && border_index(-1, 2, 0) == 1 && border_index(2, 2, 0) == 0 && border_index(-2, 2, 0) == 0,
         "reflect-101 pinned by hand");
}

static void taps()
{
  uint16_t t[8];
  for (int k : { 3, 5, 7 }) {
    VCHECK(gaussian_taps_q8(k, 0.0, t) && !std::memcmp(t, taps_of(k), sizeof(uint16_t) * k), "fixed table %d", k);
    for (double sigma : { 1e-300, 1e-3, 0.3, 0.5, 0.8, 1.0, 1.4, 2.0, 5.0, 1e3, 1e300 }) {
      bool ok = gaussian_taps_q8(k, sigma, t);
      unsigned sum = 0;
      for (int i = 0; ok && i < k; ++i) { sum += t[i]; ok = t[i] <= 256 && t[i] == t[k - 1 - i]; }
      VCHECK(ok && sum == 256 && !plan_gaussian_blur(9, 9, 1, View{ 0x1000, 9, 81 }, View{ 0x2000, 9, 81 }, 1, k, t, 0).error, "taps of ksize %d sigma %g", k, sigma);
    }
  }
  std::memset(t, 0xAB, sizeof t);
  VCHECK(!gaussian_taps_q8(4, 1.0, t) && !gaussian_taps_q8(3, NAN, t) && !gaussian_taps_q8(3, INFINITY, t) && !gaussian_taps_q8(3, -INFINITY, t) && !gaussian_taps_q8(3, 1.0, nullptr) && t[0] == 0xABAB && t[7] == 0xABAB, "taps: refusals write nothing");
}

int main()
{
  counts_and_flags();
  refusals();
  view_ends();
  overlap_by_view_end();
  borders();
  taps();
  if (g_fail) { std::printf("%ld violations in %ld checks\n", g_fail, g_checks); return 1; }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
