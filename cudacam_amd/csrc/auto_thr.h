// auto_thr.h -- the two automatic threshold rules of hc_auto_thresholds_device, from the 256-bin histogram of a u8 frame.
// Plain C++ (no HIP), host and device: k_auto_thr (stats.hip) evaluates these functions with a wave per frame, the CPU test
// compiles them into tests/cpp/auto_thr_driver.cpp and compares with the numpy restatement tests/auto_thr_ref.py.
// The pairs come out in the units of hc_set_thresholds, (low, high), as hc_frame_thresholds_device reads them.
//
//   HC_AUTO_MEDIAN, param = sigma in [0, 1]: with the N samples sorted, a = s[(N - 1) / 2], b = s[N / 2], v = (a + b) / 2.0
//     (np.median, exact in double); low = (int)max(0.0, (1.0 - sigma) * v), high = (int)min(255.0, (1.0 + sigma) * v).
//   HC_AUTO_OTSU, param = ratio in [0, 1]: N = sum h[i], S = sum i h[i]; for t = 0 .. 254, in int64, w0 = sum_{i <= t} h[i],
//     w1 = N - w0, s0 = sum_{i <= t} i h[i], d = S w0 - N s0 (exact for N <= 2^27: |d| < 2^62);
//     score(t) = ((double)d * (double)d) / ((double)w0 * (double)w1), every operation rounded once; t* = the smallest t with
//     w0, w1 > 0 whose score is strictly the largest, 0 if no t has w0, w1 > 0 (a flat frame); high = t*, low = (int)(ratio * t*).
//     This is the textbook rule (maximal between-class variance) with an exact integer numerator, stated here; it is NOT
//     pinned against OpenCV's getThreshVal_Otsu_8u, which accumulates in floating point and may pick another t at near-ties
//     -- as all of Mode O is restated from the published algorithm and not pinned against a build of OpenCV.
//
// Floating point: contraction is off (the library and the test driver are built with -ffp-contract=off; no expression below
// has the a * b + c shape anyway) and every double operation is its own statement, so host and device round alike.
#pragma once
#include "canny_params.h"

namespace hc {

constexpr int AUTO_MEDIAN = 0, AUTO_OTSU = 1;  // HC_AUTO_MEDIAN / HC_AUTO_OTSU (include/hipcanny.h)
constexpr long long AUTO_MAX_SAMPLES = 1ll << 27;  // samples per frame up to which Otsu's int64 numerator is exact

// ---- median ------------------------------------------------------------------------------------
// is sorted sample k (0-based) in the bin whose exclusive / inclusive cumulative counts are below / upto?
HC_HOST_DEVICE inline bool auto_bin_holds(long long below, long long upto, long long k) { return below <= k && k < upto; }
// a, b: the bins of samples (N - 1) / 2 and N / 2
HC_HOST_DEVICE inline void auto_median_pair(int a, int b, double sigma, int *low, int *high)
{
  const double sum = (double)a + (double)b;
  const double v = sum / 2.0;
  const double fl = 1.0 - sigma;
  const double fh = 1.0 + sigma;
  const double pl = fl * v;
  const double ph = fh * v;
  const double cl = pl < 0.0 ? 0.0 : pl;
  const double ch = ph > 255.0 ? 255.0 : ph;
  *low = (int)cl;
  *high = (int)ch;
}

// ---- Otsu --------------------------------------------------------------------------------------
// score of threshold t from the sums up to and including bin t; the caller has checked w0 > 0 and N - w0 > 0
HC_HOST_DEVICE inline double auto_otsu_score(long long N, long long S, long long w0, long long s0)
{
  const long long w1 = N - w0;
  const long long d = S * w0 - N * s0;
  const double dd = (double)d;
  const double num = dd * dd;
  const double a = (double)w0;
  const double b = (double)w1;
  const double den = a * b;
  return num / den;
}
// does (score, t) replace the best so far?  Strictly larger, or the same score at a smaller t (no best yet: best_t < 0)
HC_HOST_DEVICE inline bool auto_otsu_takes(double score, int t, double best, int best_t)
{
  return best_t < 0 || score > best || (score == best && t < best_t);
}
// t: t*, or < 0 when no threshold splits the samples
HC_HOST_DEVICE inline void auto_otsu_pair(int t, double ratio, int *low, int *high)
{
  const int ts = t < 0 ? 0 : t;
  const double pl = ratio * (double)ts;
  *low = (int)pl;
  *high = ts;
}

HC_HOST_DEVICE inline bool auto_param_ok(int rule, double param)
{
  return (rule == AUTO_MEDIAN || rule == AUTO_OTSU) && param >= 0.0 && param <= 1.0;  // (a NaN fails both comparisons)
}

// The whole rule, one bin after the other (the test driver; k_auto_thr spreads the same steps over the lanes of a wave).
inline void auto_thresholds_of_histogram(const u32 h[256], int rule, double param, int *low, int *high)
{
  long long N = 0, S = 0;
  for (int i = 0; i < 256; ++i) { N += h[i]; S += (long long)i * h[i]; }
  if (rule == AUTO_MEDIAN) {
    int a = 0, b = 0;
    long long below = 0;
    for (int i = 0; i < 256; ++i) {
      const long long upto = below + h[i];
      if (auto_bin_holds(below, upto, (N - 1) / 2)) a = i;
      if (auto_bin_holds(below, upto, N / 2)) b = i;
      below = upto;
    }
    auto_median_pair(a, b, param, low, high);
    return;
  }
  long long w0 = 0, s0 = 0;
  double best = 0.0;
  int best_t = -1;
  for (int t = 0; t < 255; ++t) {
    w0 += h[t]; s0 += (long long)t * h[t];
    if (w0 <= 0 || N - w0 <= 0) continue;
    const double score = auto_otsu_score(N, S, w0, s0);
    if (auto_otsu_takes(score, t, best, best_t)) { best = score; best_t = t; }
  }
  auto_otsu_pair(best_t, param, low, high);
}

}  // namespace hc
