// morph_plan_driver.cpp -- plan_morphology, morph_pass and structuring_spans of cudacam_amd/csrc/host_plan.h, checked without a
// GPU (tests/test_morph_plan_cpu.py builds this with g++ under ASan + UBSan): the item counts at strip and chunk boundaries, the
// alignment flags, the levels of an element, every refusal hc_morphology_device documents, the frame limits by channels /
// per_channel, overlapping and touching views, the launches of every operation, and the passes of OPEN / CLOSE at scratch bounds
// of exactly k frames, one byte less, and below one frame.
// Prints "ok <checks>" or the first violations.
//   morph_plan_driver plan W H context_channels per_channel max_batch { nframes channels op ksize span0 .. span6 in in_pitch
//                                                                       in_frame_stride out out_pitch out_frame_stride scratch_bound }...
// prints, for each group of eighteen, "scratch_bytes passes frames_per_pass" or "refused: <text>" (tests/
// test_device_op_sequences_cpu.py: the morph steps of the seeded chains).  in and out are addresses, so that the plan sees how the
// two views lie to each other; of the seven spans the first ksize count; a scratch_bound of 0 is the context's default, as
// hc_set_option takes it.
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace hc;

static long g_checks = 0, g_fail = 0;
#define VCHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL "); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const size_t BIG = (size_t)256 << 20;
static const int8_t R3[3] = { 1, 1, 1 }, R5[5] = { 2, 2, 2, 2, 2 }, R7[7] = { 3, 3, 3, 3, 3, 3, 3 };
static const int8_t *rect_of(int k) { return k == 3 ? R3 : k == 5 ? R5 : R7; }

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
              const int mop = bits % 5;
              const MorphPlan P = plan_morphology(W, H, 3, false, 5, in, out, n, C, mop, k, rect_of(k), BIG);
              const MorphParams &m = P.mp;
              const int strips = (W + BLUR_STRIP_W - 1) / BLUR_STRIP_W, chunks = (H + BLUR_CHUNK_ROWS - 1) / BLUR_CHUNK_ROWS;
              VCHECK(!P.error && m.nstrips == strips && m.nchunks == chunks && m.total_items == n * strips * chunks && P.passes == 1 && P.frames_per_pass == n, "%d x %d x %d n %d: %d strips, %d chunks, %d items (%s)",
                     W, H, C, n, m.nstrips, m.nchunks, m.total_items, P.error ? P.error : "");
              VCHECK((m.in_aligned != 0) == ((bits & 0x15) == 0) && (m.out_aligned != 0) == ((bits & 0x2A) == 0), "%d x %d x %d bits %x: in_aligned %d out_aligned %d", W, H, C, bits, m.in_aligned, m.out_aligned);
              VCHECK(m.in == (const uint8_t *)in.p && m.in_pitch == ip && m.in_frame_stride == ifs && m.out == (uint8_t *)out.p && m.out_pitch == op && m.out_frame_stride == ofs && m.W == W && m.H == H
                     && m.nframes == n && m.channels == C && m.ksize == k && !m.complement && !m.subtract, "%d x %d x %d n %d: views", W, H, C, n);
              VCHECK(m.nlevels == 1 && m.level[0] == k / 2, "%d: a RECT has one level", k);
              VCHECK(P.stages == (mop == MORPH_ERODE || mop == MORPH_DILATE ? 1 : 2) && (P.scratch_bytes != 0) == (mop == MORPH_OPEN || mop == MORPH_CLOSE), "op %d: stages %d scratch %zu", mop, P.stages, P.scratch_bytes);
              if (P.scratch_bytes) VCHECK(P.scratch_pitch == (row + 3) / 4 * 4 && P.scratch_frame_bytes == P.scratch_pitch * H && P.scratch_bytes == P.scratch_frame_bytes * n, "%d x %d x %d: scratch layout", W, H, C);
            }
  // pinned by hand: 1080p, 512 maps: 8 strips x 17 chunks
  const View in{ 0x10000000u, 1920, 1920 * 1080 }, out{ 0x50000000u, 1920, 1920 * 1080 };
  const MorphPlan P = plan_morphology(1920, 1080, 1, false, 512, in, out, 512, 1, MORPH_DILATE, 5, R5, BIG);
  VCHECK(!P.error && P.mp.nstrips == 8 && P.mp.nchunks == 17 && P.mp.total_items == 512 * 8 * 17 && P.mp.in_aligned && P.mp.out_aligned, "pinned 1080p plan");
}

static void levels()
{
  const int W = 20, H = 10;
  const View in{ 0x1000, 20, 200 }, out{ 0x9000, 20, 200 };
  struct { int k; int8_t s[7]; int nlev; int8_t lev[4]; int8_t rl[7]; } cases[] = {
    { 3, { 0, 1, 0 }, 2, { 0, 1 }, { 0, 1, 0 } },
    { 3, { 1, 0, -1 }, 2, { 0, 1 }, { 1, 0, -1 } },
    { 3, { -1, 0, -1 }, 1, { 0 }, { -1, 0, -1 } },
    { 5, { 0, 2, 2, 2, 0 }, 2, { 0, 2 }, { 0, 1, 1, 1, 0 } },
    { 5, { 2, 1, 0, -1, 1 }, 3, { 0, 1, 2 }, { 2, 1, 0, -1, 1 } },
    { 7, { 0, 2, 3, 3, 3, 2, 0 }, 3, { 0, 2, 3 }, { 0, 1, 2, 2, 2, 1, 0 } },
    { 7, { -1, 0, 3, 1, 2, 0, 3 }, 4, { 0, 1, 2, 3 }, { -1, 0, 3, 1, 2, 0, 3 } },
    { 7, { 2, -1, -1, -1, -1, -1, -1 }, 1, { 2 }, { 0, -1, -1, -1, -1, -1, -1 } },
  };
  for (const auto &c : cases) {
    const MorphPlan P = plan_morphology(W, H, 1, false, 4, in, out, 1, 1, MORPH_ERODE, c.k, c.s, BIG);
    bool ok = !P.error && P.mp.nlevels == c.nlev;
    for (int l = 0; ok && l < MORPH_MAX_LEVELS; ++l) ok = P.mp.level[l] == (l < c.nlev ? c.lev[l] : 0);
    for (int j = 0; ok && j <= MORPH_MAX_K; ++j) ok = P.mp.row_level[j] == (j < c.k ? c.rl[j] : -1);
    VCHECK(ok, "levels of a %d-row element starting %d %d %d", c.k, c.s[0], c.s[1], c.s[2]);
  }
  // structuring_spans: the pinned tables; refusals write nothing
  const int8_t want[3][3][7] = { { { 1, 1, 1 }, { 2, 2, 2, 2, 2 }, { 3, 3, 3, 3, 3, 3, 3 } },
                                 { { 0, 1, 0 }, { 0, 0, 2, 0, 0 }, { 0, 0, 0, 3, 0, 0, 0 } },
                                 { { 0, 1, 0 }, { 0, 2, 2, 2, 0 }, { 0, 2, 3, 3, 3, 2, 0 } } };
  for (int shape = 0; shape < 3; ++shape)
    for (int ki = 0; ki < 3; ++ki) {
      int8_t s[8];
      std::memset(s, 77, sizeof s);
      const int k = 3 + 2 * ki;
      VCHECK(structuring_spans(shape, k, s) && !std::memcmp(s, want[shape][ki], (size_t)k) && s[k] == 77, "structuring_spans(%d, %d)", shape, k);
    }
  int8_t s[8];
  std::memset(s, 77, sizeof s);
  bool wrote = false;
  for (int shape : { -1, 3, 99 }) wrote = wrote || structuring_spans(shape, 3, s);
  for (int k : { -3, 0, 1, 2, 4, 6, 8, 9 }) wrote = wrote || structuring_spans(HC_MORPH_ELLIPSE, k, s);
  wrote = wrote || structuring_spans(HC_MORPH_RECT, 3, nullptr);
  for (int i = 0; i < 8; ++i) wrote = wrote || s[i] != 77;
  VCHECK(!wrote, "structuring_spans: refusals write nothing");
}

static void refusals()
{
  const int W = 64, H = 32;
  const size_t row3 = (size_t)W * 3, row1 = (size_t)W;
  const View in{ 0x10000000u, row3, row3 * H }, out{ 0x20000000u, row3 + 4, (row3 + 4) * H };
  auto plan = [&](const View &i, const View &o, int n, int ch, int op, int k, const int8_t *s, int ctxC = 3, bool pc = false, int mb = 4, size_t bound = BIG) {
    return plan_morphology(W, H, ctxC, pc, mb, i, o, n, ch, op, k, s, bound);
  };
  auto refused = [](const MorphPlan &P) { return P.error && !P.passes && !P.stages && !P.mp.in && !P.mp.out && !P.mp.total_items && !P.scratch_bytes; };
  for (int op = 0; op < 5; ++op) VCHECK(!plan(in, out, 2, 3, op, 3, R3).error && !plan(in, out, 1, 1, op, 7, R7).error && !plan(in, out, 4, 1, op, 5, R5, 1).error, "the valid calls, op %d", op);
  VCHECK(refused(plan(View{ 0, row3, row3 * H }, out, 1, 3, 1, 3, R3)) && refused(plan(in, View{ 0, row3, row3 * H }, 1, 3, 1, 3, R3)) && refused(plan(in, out, 1, 3, 1, 3, nullptr)), "null pointers");
  for (int ch : { -1, 0, 2, 4 }) VCHECK(refused(plan(in, out, 1, ch, 1, 3, R3)), "channels %d", ch);
  VCHECK(refused(plan(in, out, 1, 3, 1, 3, R3, 1)) && std::strstr(plan(in, out, 1, 3, 1, 3, R3, 1).error, "3-channel context"), "channels 3 on a one-channel context");
  for (int op : { -1, 5, 6, 100 }) VCHECK(refused(plan(in, out, 1, 3, op, 3, R3)), "op %d", op);
  for (int k : { -1, 0, 1, 2, 4, 6, 8, 9 }) VCHECK(refused(plan(in, out, 1, 3, 1, k, R7)), "ksize %d", k);
  for (int k : { 3, 5, 7 })
    for (int j = 0; j < k; ++j)
      for (int v : { -128, -2, k / 2 + 1, 127 }) {
        int8_t s[7];
        std::memcpy(s, rect_of(k), (size_t)k);
        s[j] = (int8_t)v;
        VCHECK(refused(plan(in, out, 1, 3, 1, k, s)), "ksize %d span[%d] = %d", k, j, v);
        s[j] = -1;
        VCHECK(!plan(in, out, 1, 3, 1, k, s).error, "ksize %d span[%d] = -1 is an empty row", k, j);
      }
  const int8_t E7[7] = { -1, -1, -1, -1, -1, -1, -1 };
  for (int k : { 3, 5, 7 }) VCHECK(refused(plan(in, out, 1, 3, 1, k, E7)) && std::strstr(plan(in, out, 1, 3, 1, k, E7).error, "empty"), "all rows empty, ksize %d", k);
  VCHECK(refused(plan(View{ in.p, row3 - 1, row3 * H }, out, 1, 3, 1, 3, R3)) && refused(plan(in, View{ out.p, row3 - 1, (row3 + 4) * H }, 1, 3, 1, 3, R3)), "pitch below a row");
  VCHECK(!plan(View{ in.p, row1, row1 * H }, out, 1, 1, 1, 3, R3).error && refused(plan(View{ in.p, row1 - 1, row1 * H }, out, 1, 1, 1, 3, R3)), "the row is channels * width: the caller's channels");
  VCHECK(refused(plan(in, out, 0, 3, 1, 3, R3)) && refused(plan(in, out, -1, 3, 1, 3, R3)), "nframes < 1");
  // the frame limits: channels = 3: max_batch; channels = 1: max_batch, 3 * max_batch on a per-channel context
  VCHECK(!plan(in, out, 4, 3, 1, 3, R3).error && refused(plan(in, out, 5, 3, 1, 3, R3)), "3 channels: max_batch frames");
  VCHECK(!plan(in, out, 4, 3, 1, 3, R3, 3, true).error && refused(plan(in, out, 5, 3, 1, 3, R3, 3, true)), "3 channels on a per-channel context: max_batch frames");
  VCHECK(!plan(in, out, 4, 1, 1, 3, R3).error && refused(plan(in, out, 5, 1, 1, 3, R3)) && !plan(in, out, 4, 1, 1, 3, R3, 1).error && refused(plan(in, out, 5, 1, 1, 3, R3, 1)), "1 channel: max_batch maps");
  VCHECK(!plan(in, out, 12, 1, 1, 3, R3, 3, true).error && refused(plan(in, out, 13, 1, 1, 3, R3, 3, true)) && std::strstr(plan(in, out, 13, 1, 1, 3, R3, 3, true).error, "nframes out of range"), "1 channel on a per-channel context: 3 * max_batch maps");
  VCHECK(refused(plan(View{ in.p, row3, row3 * H - 1 }, out, 2, 3, 1, 3, R3)) && !plan(View{ in.p, row3, row3 * H - 1 }, out, 1, 3, 1, 3, R3).error && refused(plan(in, View{ out.p, row3 + 4, (row3 + 4) * H - 1 }, 2, 3, 1, 3, R3)),
         "a frame stride below height * pitch at n = 2, not at n = 1");
  const size_t huge = ((size_t)1 << 32) / H;  // H * pitch = 2^32
  VCHECK(refused(plan(View{ in.p, huge, huge * H }, out, 1, 3, 1, 3, R3)) && refused(plan(in, View{ out.p, huge, huge * H }, 1, 3, 1, 3, R3)) && !plan(View{ in.p, huge - 1, (huge - 1) * H }, View{ 0x100000000000ull, row3, row3 * H }, 1, 3, 1, 3, R3).error,
         "height * pitch >= 2^32");
  VCHECK(refused(plan(View{ UINTPTR_MAX - 100, row3, row3 * H }, out, 1, 3, 1, 3, R3)), "a view that wraps the address space");
  // overlap: in place, one shared byte on either side; views that touch pass
  const size_t bytes2 = row3 * H + (H - 1) * row3 + row3;  // n = 2 at stride row3 * H: 2 * row3 * H
  VCHECK(refused(plan(in, View{ in.p, row3, row3 * H }, 1, 3, 1, 3, R3)), "in place");
  VCHECK(refused(plan(in, View{ in.p + bytes2 - 1, row3, row3 * H }, 2, 3, 1, 3, R3)) && !plan(in, View{ in.p + bytes2, row3, row3 * H }, 2, 3, 1, 3, R3).error, "the output begins on / behind the input's last byte");
  VCHECK(refused(plan(View{ out.p + 1, row3, row3 * H }, View{ out.p + 2 - bytes2, row3, row3 * H }, 2, 3, 1, 3, R3)) && !plan(View{ out.p, row3, row3 * H }, View{ out.p - bytes2, row3, row3 * H }, 2, 3, 1, 3, R3).error,
         "the output ends on / before the input's first byte");
  for (int op : { MORPH_OPEN, MORPH_CLOSE }) {
    const MorphPlan P = plan(in, out, 1, 3, op, 3, R3, 3, false, 4, row3 * H - 1);
    VCHECK(refused(P) && std::strstr(P.error, "scratch bound"), "one frame above the scratch bound, op %d", op);
  }
  for (int op : { MORPH_ERODE, MORPH_DILATE, MORPH_GRADIENT }) VCHECK(!plan(in, out, 4, 3, op, 3, R3, 3, false, 4, 1).error, "op %d needs no scratch: any bound", op);
}

static void passes()
{
  // W = 61, 3 channels: rows of 183 bytes, the scratch pitch 184
  const int W = 61, H = 9, n = 4;
  const size_t row = 183, sp = 184, frame = sp * H;
  const View in{ 0x10000001u, row + 2, (row + 2) * H + 7 }, out{ 0x20000003u, row, row * H + 1 };
  const int8_t S[3] = { 1, 0, -1 };
  const uintptr_t scratch = 0x70000000u;
  for (int op = 0; op < 5; ++op) {
    const bool two = op == MORPH_OPEN || op == MORPH_CLOSE;
    struct { size_t bound; int fpp, passes; } cases[] = { { BIG, 4, 1 }, { 4 * frame, 4, 1 }, { 4 * frame - 1, 3, 2 }, { 3 * frame, 3, 2 }, { 2 * frame, 2, 2 }, { 2 * frame - 1, 1, 4 }, { frame, 1, 4 } };
    for (const auto &c : cases) {
      const MorphPlan P = plan_morphology(W, H, 3, false, n, in, out, n, 3, op, 3, S, c.bound);
      const int fpp = two ? c.fpp : n, np = two ? c.passes : 1;
      VCHECK(!P.error && P.frames == n && P.frames_per_pass == fpp && P.passes == np && P.scratch_bytes == (two ? (size_t)fpp * frame : 0) && P.scratch_pitch == (two ? sp : 0), "op %d bound %zu: %d frames per pass, %d passes (%s)", op,
             c.bound, P.frames_per_pass, P.passes, P.error ? P.error : "");
      if (P.error) continue;
      int seen = 0;
      for (int k = 0; k < P.passes; ++k) {
        const MorphPass M = morph_pass(P, k, scratch);
        const int f0 = k * fpp, nf = std::min(fpp, n - f0);
        const MorphParams &a = M.st[0], &b = M.st[1];
        VCHECK(M.stages == P.stages && a.nframes == nf && a.total_items == nf * a.nstrips * a.nchunks && a.in == (const uint8_t *)in.p + (size_t)f0 * in.fs && a.in_pitch == in.pitch && a.in_frame_stride == in.fs && !a.in_aligned,
               "op %d pass %d: the first launch reads the caller's frames %d ..", op, k, f0);
        const MorphParams &last = M.st[M.stages - 1];
        VCHECK(last.nframes == nf && last.out == (uint8_t *)out.p + (size_t)f0 * out.fs && last.out_pitch == out.pitch && last.out_frame_stride == out.fs && !last.out_aligned, "op %d pass %d: the last launch writes the caller's frames", op, k);
        if (op == MORPH_ERODE) VCHECK(a.complement && !a.subtract, "erode: the complement");
        if (op == MORPH_DILATE) VCHECK(!a.complement && !a.subtract, "dilate: plain");
        if (op == MORPH_GRADIENT)
          VCHECK(!a.complement && !a.subtract && a.out == b.out && b.complement && b.subtract && b.in == a.in && b.in_pitch == in.pitch && b.total_items == a.total_items, "gradient: dilate, then erode subtracted in place");
        if (two) {
          VCHECK(a.complement == (op == MORPH_OPEN) && b.complement == (op == MORPH_CLOSE) && !a.subtract && !b.subtract, "op %d: the order of the stages", op);
          VCHECK(a.out == (uint8_t *)scratch && a.out_pitch == sp && a.out_frame_stride == frame && a.out_aligned && b.in == (const uint8_t *)scratch && b.in_pitch == sp && b.in_frame_stride == frame && b.in_aligned
                 && b.nframes == nf && b.total_items == a.total_items && (size_t)nf * frame <= P.scratch_bytes, "op %d pass %d: through the scratch, inside it", op, k);
        }
        seen += nf;
      }
      VCHECK(seen == n, "op %d bound %zu: the passes cover %d of %d frames", op, c.bound, seen, n);
    }
    const MorphPlan R = plan_morphology(W, H, 3, false, n, in, out, n, 3, op, 3, S, frame - 1);
    VCHECK(two ? (R.error && std::strstr(R.error, "scratch bound") && !R.passes) : !R.error, "op %d: a bound one byte below one frame", op);
  }
}

static int print_plans(int count, char **v)
{
  const int W = std::atoi(v[0]), H = std::atoi(v[1]), ctxC = std::atoi(v[2]), mb = std::atoi(v[4]);
  const bool pc = std::atoi(v[3]) != 0;
  auto num = [](const char *t) { return (size_t)std::strtoull(t, nullptr, 10); };
  for (char **g = v + 5; g + 18 <= v + count; g += 18) {
    int8_t spans[7];
    for (int j = 0; j < 7; ++j) spans[j] = (int8_t)std::atoi(g[4 + j]);
    const View in{ (uintptr_t)num(g[11]), num(g[12]), num(g[13]) }, out{ (uintptr_t)num(g[14]), num(g[15]), num(g[16]) };
    const size_t bound = num(g[17]);
    const MorphPlan P = plan_morphology(W, H, ctxC, pc, mb, in, out, std::atoi(g[0]), std::atoi(g[1]), std::atoi(g[2]), std::atoi(g[3]), spans, bound ? bound : HOUGH_SCRATCH_BYTES);
    if (P.error) std::printf("refused: %s\n", P.error);
    else std::printf("%zu %d %d\n", P.scratch_bytes, P.passes, P.frames_per_pass);
  }
  return 0;
}

int main(int argc, char **argv)
{
  if (argc >= 7 && (argc - 7) % 18 == 0 && !std::strcmp(argv[1], "plan")) return print_plans(argc - 2, argv + 2);
  counts_and_flags();
  levels();
  refusals();
  passes();
  if (g_fail) {
    std::printf("%ld of %ld checks failed\n", g_fail, g_checks);
    return 1;
  }
  std::printf("ok %ld\n", g_checks);
  return 0;
}
