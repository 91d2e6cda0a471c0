// auto_thr_driver.cpp -- the host-callable parts of the per-frame / automatic thresholds without a GPU
// (tests/test_auto_thr_cpu.py builds this with g++ under ASan + UBSan against cudacam_amd/csrc).
//   auto_thr_driver hist FILE    one "rule param h0 .. h255" per line -> "low high" per line (auto_thresholds_of_histogram,
//                                auto_thr.h), or "refused" when auto_param_ok says no
//   auto_thr_driver pairs FILE   one "low high l2" per line -> "a_lo a_hi p_lo p_hi": frame_threshold_pair (canny_params.h),
//                                and what plan_front puts into a_lo[0] / a_hi[0] for a context whose thresholds were set to
//                                the same pair (set_thresholds below restates hc_set_thresholds for a mode O context)
//   auto_thr_driver plans        front plans of both modes on the shapes of tests/cpp/plan_driver.cpp's option product; no
//                                plan sets FrontParams::frame_thr; prints "ok <plans> <FNV-1a digest of every other field>"
#include "../../cudacam_amd/csrc/auto_thr.h"
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace hc;

static int hist(const char *path)
{
  FILE *f = std::fopen(path, "r");
  if (!f) return 2;
  static char line[8192];
  while (std::fgets(line, sizeof line, f)) {
    char *p = line;
    const long rule = std::strtol(p, &p, 10);
    const double param = std::strtod(p, &p);
    u32 h[256];
    for (int i = 0; i < 256; ++i) h[i] = (u32)std::strtoul(p, &p, 10);
    if (!auto_param_ok((int)rule, param)) { std::printf("refused\n"); continue; }
    int low = -1, high = -1;
    auto_thresholds_of_histogram(h, (int)rule, param, &low, &high);
    std::printf("%d %d\n", low, high);
  }
  std::fclose(f);
  return 0;
}

// hc_set_thresholds on a mode O context (hipcanny.hip)
static void set_thresholds(FrontOpts &o, int low, int high)
{
  low = std::max(0, std::min(32767, low));
  high = std::max(0, std::min(32767, high));
  if (low > high) std::swap(low, high);
  o.low = low; o.high = high;
}

static FrontIn make_in(int mode, int C, int W, int H, int n, bool piped, const FrontOpts &o, bool grads)
{
  FrontIn fi{ mode, C, W, H, plane_row_dwords(W), (W + STRIP_W - 1) / STRIP_W, 0, HC_STAGE_HYSTER, n };
  const size_t row = grads ? (size_t)2 * W * C : round_up((size_t)W, 8) * C;
  fi.in = View{ 0x10000000u, row, row * H }; fi.out = View{ 0x20000000u, round_up((size_t)W, 4), round_up((size_t)W, 4) * H };
  fi.in_dy = grads ? 0x30000000u : 0;
  fi.own_in.pitch = frame_pitch(round_up((size_t)W, 8) * C, (size_t)W * C); fi.own_in.fs = fi.own_in.pitch * H; fi.own_in.p = 0;
  fi.own_out.pitch = frame_pitch((size_t)W, (size_t)W); fi.own_out.fs = fi.own_out.pitch * H; fi.own_out.p = 0;
  fi.own_mono.pitch = frame_pitch((size_t)W, 0); fi.own_mono.fs = fi.own_mono.pitch * H; fi.own_mono.p = 0;
  fi.o = o; fi.dump_region = 0; fi.piped = piped; fi.nslot_use = piped ? pipeline_slots(0, 2, n, W, H) : 2;
  fi.front_one = false; fi.out_overlap = false; fi.wl_cap = slot_wl_cap((size_t)n, H, fi.RD);
  return fi;
}

static int pairs(const char *path)
{
  FILE *f = std::fopen(path, "r");
  if (!f) return 2;
  char line[256];
  while (std::fgets(line, sizeof line, f)) {
    char *p = line;
    const long low = std::strtol(p, &p, 10), high = std::strtol(p, &p, 10), l2 = std::strtol(p, &p, 10);
    u32 a_lo = 1, a_hi = 1;
    frame_threshold_pair((int)low, (int)high, (int)l2, &a_lo, &a_hi);
    FrontOpts o;
    set_thresholds(o, (int)low, (int)high);
    o.l2gradient = l2 != 0;
    const FrontPlan P = plan_front(make_in(HC_MODE_O, 1, 64, 48, 1, false, o, false));
    if (P.error || P.fp.frame_thr) { std::printf("plan error\n"); continue; }
    std::printf("%u %u %u %u\n", a_lo, a_hi, P.fp.a_lo[0], P.fp.a_hi[0]);
  }
  std::fclose(f);
  return 0;
}

// ---- plans: FNV-1a over every field of every plan but frame_thr, which must be null ----------------------------------
static unsigned long long g_digest = 0xcbf29ce484222325ull;
static long g_plans = 0, g_fail = 0;
static void fold_byte(unsigned b) { g_digest = (g_digest ^ (b & 0xFFu)) * 0x100000001b3ull; }
template <class T> static void fold(T v)
{
  unsigned long long u = (unsigned long long)v;
  for (unsigned k = 0; k < sizeof(T); ++k) fold_byte((unsigned)(u >> (8 * k)));
}
template <class T> static void fold(T *p) { fold((uintptr_t)p); }
static void fold(bool b) { fold_byte(b ? 1 : 0); }
static void fold(const char *s) { for (; s && *s; ++s) fold_byte((unsigned char)*s); fold_byte(0); }
static void fold(const View &v) { fold(v.p); fold(v.pitch); fold(v.fs); }
static void fold(const FrontPlan &P)
{
  const FrontParams &f = P.fp;
  fold(P.error); fold(P.in_staged); fold(P.out_staged); fold(P.gray); fold(P.src); fold(P.mono); fold(P.dst);
  fold(P.form); fold(P.prov); fold(P.zeroed_words); fold(P.waves); fold(P.mask); fold(P.mask_a);
  fold(f.in); fold(f.bgr); fold(f.in_pitch); fold(f.in_frame_stride); fold(f.sbits); fold(f.cbits); fold(f.RD); fold(f.W); fold(f.H);
  fold(f.nstrips); fold(f.nchunks); fold(f.nframes); fold(f.subchunks); fold(f.run_rows);
  fold(f.chunk_rows); fold(f.l2gradient); fold(f.total_items);
  for (int k = 0; k < 3; ++k) { fold(f.a_lo[k]); fold(f.a_hi[k]); }
  fold(f.blur); fold(f.blur_frame_stride); fold(f.nchunks_b); fold(f.run_rows_b); fold(f.total_items_b);
  fold(f.prov_out); fold(f.prov_pitch); fold(f.prov_fs); fold(f.dbg_blur); fold(f.dbg_pitch); fold(f.dbg_fs);
  fold(f.zeros); fold(f.dump); fold(f.dump_c); fold(f.dump_p); fold(f.zero_words); fold(f.zero_count);
  fold(f.half); fold(f.one_wave); fold(f.nhalf); fold(f.dense_enter); fold(f.dense_leave); fold(f.wrap_limit);
  if (f.frame_thr != nullptr) ++g_fail;  // (no plan installs a table: the launcher patches the pointer in)
  ++g_plans;
}

static int plans()
{
  const int sizes[] = { 1, 7, 8, 16, 239, 240, 241, 247, 248, 249, 480, 495, 496, 497, 1079, 1080, 2160, 4320 };
  for (int W : sizes)
    for (int H : sizes)
      for (int mode : { HC_MODE_R, HC_MODE_O })
        for (int C : { 1, 3 })
          for (int n : { 1, 8, 1024 })
            for (int piped = 0; piped <= 1; ++piped)
              for (int chunk : { 0, 1, 7, 300 })
                for (int variant = 0; variant < 4; ++variant) {
                  if ((long long)W * H * n > (1ll << 31)) continue;
                  FrontOpts o;
                  o.chunk = chunk;
                  bool grads = false;
                  if (mode == HC_MODE_O) {
                    set_thresholds(o, 50 + W, 150 + H);
                    o.l2gradient = variant & 1;
                    if (variant == 2) o.aperture = 5;
                    if (variant == 3) grads = true;
                  } else {
                    o.low = 10 + W % 200; o.high = 40 + H % 200;
                    o.nms_saturate = variant & 1;
                    o.debug_taps = (variant & 2) != 0;
                  }
                  fold(plan_front(make_in(mode, C, W, H, n, piped != 0, o, grads)));
                }
  if (g_fail) { std::printf("%ld plans carry a threshold table\n", g_fail); return 1; }
  std::printf("ok %ld %016llx\n", g_plans, g_digest);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "hist")) return hist(argv[2]);
  if (argc == 3 && !std::strcmp(argv[1], "pairs")) return pairs(argv[2]);
  if (argc == 2 && !std::strcmp(argv[1], "plans")) return plans();
  std::printf("usage: auto_thr_driver hist FILE | pairs FILE | plans\n");
  return 2;
}
