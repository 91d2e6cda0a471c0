// canny_call_driver.cpp -- hc_canny_device's host side without a GPU (tests/test_canny_call_cpu.py builds this with g++ under
// ASan + UBSan against cudacam_amd/csrc/host_plan.h).
//   canny_call_driver thresholds FILE   one "low high aperture l2" per line (strtod: "nan", "inf" and hex floats parse) ->
//                                       "lo hi k_lo k_hi" per line, or "refused" (canny_call_thresholds)
//   canny_call_driver plans             plans of apertures 7 / -1 beside aperture 5 and the gradient form on the same inputs;
//                                       prints "plan <aperture> <C> <piped> <set rows> <form> <chunk_rows> <nchunks> <total_items>" lines (322 x 97, one frame) and
//                                       "ok <plans>", or the first violations
#include "../../cudacam_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace hc;

static int thresholds(const char *path)
{
  FILE *f = std::fopen(path, "r");
  if (!f) return 2;
  char line[512];
  while (std::fgets(line, sizeof line, f)) {
    char *p = line;
    const double low = std::strtod(p, &p), high = std::strtod(p, &p);
    const long aperture = std::strtol(p, &p, 10), l2 = std::strtol(p, &p, 10);
    CallThresholds t;
    if (!canny_call_thresholds(low, high, (int)aperture, l2 != 0, &t)) std::printf("refused\n");
    else std::printf("%lld %lld %d %d\n", t.lo, t.hi, t.k_lo, t.k_hi);
  }
  std::fclose(f);
  return 0;
}

static long g_fail = 0, g_plans = 0;
#define CHECK(cond, what) do { if (!(cond)) { if (++g_fail <= 20) std::printf("FAIL %s (W %d H %d C %d n %d piped %d chunk %d aperture %d)\n", what, W, H, C, n, piped, chunk, ap); } } while (0)

static FrontIn make_in(int C, int W, int H, int n, bool piped, const FrontOpts &o, const View &in, bool grads)
{
  FrontIn fi{ HC_MODE_O, C, W, H, plane_row_dwords(W), (W + STRIP_W - 1) / STRIP_W, 0, HC_STAGE_HYSTER, n };
  fi.in = in; fi.out = View{ 0x20000000u, (size_t)W, (size_t)W * H }; fi.in_dy = grads ? 0x30000000u : 0;
  fi.own_in.pitch = frame_pitch(round_up((size_t)W, 8) * C, (size_t)W * C); fi.own_in.fs = fi.own_in.pitch * H; fi.own_in.p = 0;
  fi.own_out.pitch = frame_pitch((size_t)W, (size_t)W); fi.own_out.fs = fi.own_out.pitch * H; fi.own_out.p = 0;
  fi.own_mono.pitch = frame_pitch((size_t)W, 0); fi.own_mono.fs = fi.own_mono.pitch * H; fi.own_mono.p = 0;
  fi.o = o; fi.dump_region = 0; fi.piped = piped; fi.nslot_use = piped ? pipeline_slots(0, 2, n, W, H) : 2;
  fi.front_one = false; fi.out_overlap = false; fi.wl_cap = slot_wl_cap((size_t)n, H, fi.RD);
  return fi;
}

// every field a launch reads, but the form and the thresholds
static bool same_cut(const FrontPlan &a, const FrontPlan &b)
{
  const FrontParams &x = a.fp, &y = b.fp;
  return !a.error && !b.error && a.in_staged == b.in_staged && a.out_staged == b.out_staged && a.gray == b.gray && a.prov == b.prov && a.mask == b.mask
         && a.mask_a == b.mask_a && a.waves == b.waves && a.zeroed_words == b.zeroed_words && a.src.pitch == b.src.pitch && a.src.fs == b.src.fs
         && a.dst.pitch == b.dst.pitch && a.dst.fs == b.dst.fs && x.bgr == y.bgr && x.in_pitch == y.in_pitch && x.in_frame_stride == y.in_frame_stride
         && x.RD == y.RD && x.W == y.W && x.H == y.H && x.nstrips == y.nstrips && x.nchunks == y.nchunks && x.nframes == y.nframes
         && x.chunk_rows == y.chunk_rows && x.total_items == y.total_items && x.l2gradient == y.l2gradient && x.prov_pitch == y.prov_pitch
         && x.dbg_pitch == y.dbg_pitch && x.zero_count == y.zero_count;
}
static bool same_plan(const FrontPlan &a, const FrontPlan &b)
{
  return same_cut(a, b) && a.form == b.form && a.fp.a_lo[0] == b.fp.a_lo[0] && a.fp.a_hi[0] == b.fp.a_hi[0];
}

static int plans()
{
  const int sizes[][2] = { { 1, 1 }, { 5, 3 }, { 253, 29 }, { 322, 97 }, { 497, 10 }, { 640, 480 }, { 1920, 1080 }, { 8184, 4320 } };
  for (const auto &s : sizes)
    for (int C : { 1, 3 })
      for (int n : { 1, 8, 1024 })
        for (int piped = 0; piped <= 1; ++piped)
          for (int chunk : { 0, 1, 7, 16, 300 })
            for (int l2 = 0; l2 <= 1; ++l2) {
              const int W = s[0], H = s[1];
              if ((long long)W * H * n > (1ll << 31)) continue;
              const size_t tight = (size_t)W * C;
              const View views[] = { View{ 0x10000000u, tight, tight * H }, View{ 0x10000000u, round_up(tight, 4) + 8, (round_up(tight, 4) + 8) * H },
                                     View{ 0x10000001u, tight + 3, (tight + 3) * H } };
              for (const View &v : views) {
                FrontOpts o5; o5.aperture = 5; o5.chunk = chunk; o5.l2gradient = l2; o5.low = 100; o5.high = 300;
                int ap = 5;
                const FrontPlan P5 = plan_front(make_in(C, W, H, n, piped != 0, o5, v, false));
                CHECK(!P5.error && P5.form == HC_FORM_O_APERTURE5, "aperture 5 plans to form 6");
                // the new fields at their defaults change nothing: a call's thresholds that restate the context's give the same plan
                FrontOpts o5c = o5; o5c.call_lo = l2 ? 100 * 100 : 100; o5c.call_hi = l2 ? 300 * 300 : 300;
                CHECK(same_plan(P5, plan_front(make_in(C, W, H, n, piped != 0, o5c, v, false))), "aperture 5 with restated call thresholds");
                FrontOpts od = FrontOpts{}; od.aperture = 5; od.chunk = chunk; od.l2gradient = l2; od.low = 100; od.high = 300;
                CHECK(od.call_lo == -1 && od.call_hi == -1 && same_plan(P5, plan_front(make_in(C, W, H, n, piped != 0, od, v, false))), "defaults");
                for (int a : { 7, -1 }) {
                  ap = a;
                  FrontOpts o = o5; o.aperture = a; o.call_lo = 7; o.call_hi = 1073676289;
                  const FrontPlan P = plan_front(make_in(C, W, H, n, piped != 0, o, v, false));
                  ++g_plans;
                  CHECK(!P.error && P.form == (a == 7 ? HC_FORM_O_APERTURE7 : HC_FORM_O_SCHARR), "apertures 7 / -1 plan to forms 8 / 9");
                  CHECK(form_o_4px(P.form) && form_o_ext(P.form), "form groups");
                  CHECK(same_cut(P, P5), "cut, staging and masks as aperture 5");
                  CHECK(P.fp.a_lo[0] == 7u && P.fp.a_hi[0] == 1073676289u, "the call's thresholds reach the kernel as they are");
                  CHECK(!P.prov && P.mask == (B_GRAD | B_NMS | B_THR), "no provisional map; GRADIENT + NMS + THRESH");
                  CHECK(P.fp.chunk_rows >= 1 && (long)P.fp.nchunks * P.fp.chunk_rows >= H && P.fp.total_items == n * P.fp.nstrips * P.fp.nchunks, "items");
                  if (chunk) CHECK(P.fp.chunk_rows == std::min(chunk, H), "hc_set_tuning's rows as they are");
                  CHECK(P.fp.in_pitch % 4 == 0 && P.fp.in_pitch >= round_up((size_t)W, 4) * C && !reaches_4g(H, P.fp.in_pitch), "rows hold whole 4-pixel groups");
                  if (W == 322 && l2 == 0 && &v == &views[0] && n == 1)
                    std::printf("plan %d %d %d %d %d %d %d %d\n", a, C, piped, chunk, P.form, P.fp.chunk_rows, P.fp.nchunks, P.fp.total_items);
                }
                ap = 0;
                // the gradient form beside them: the context's aperture does not matter to it, nor do defaults
                FrontOpts og; og.chunk = chunk; og.l2gradient = l2;
                const View gv{ 0x10000000u, 2 * tight, 2 * tight * H };
                const FrontPlan G = plan_front(make_in(C, W, H, n, piped != 0, og, gv, true));
                CHECK(!G.error && G.form == HC_FORM_O_GRADIENTS && G.mask == (B_NMS | B_THR), "gradients plan to form 7");
                FrontOpts og7 = og; og7.aperture = 7;
                CHECK(same_plan(G, plan_front(make_in(C, W, H, n, piped != 0, og7, gv, true))), "gradients ignore the aperture");
              }
            }
  if (g_fail) { std::printf("%ld violations\n", g_fail); return 1; }
  std::printf("ok %ld\n", g_plans);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "thresholds")) return thresholds(argv[2]);
  if (argc == 2 && !std::strcmp(argv[1], "plans")) return plans();
  std::printf("usage: canny_call_driver thresholds FILE | plans\n");
  return 2;
}
