// sep_deriv.h -- the separable derivative row source of k_deriv16 (deriv.hip) and of k_front_o_ext's u8 sources
// (front_o_ext.hip): Sobel(src, CV_16S, 1, 0 / 0, 1, ksize, scale, 0, BORDER_REPLICATE) restated, a correlation: dx =
// derivative taps along x and smoothing taps along y, dy the other way round; the taps are smooth_tap / deriv_tap below,
// ksize 7 is scaled by 1 / 16 and rounded half to even.  KIND is cv's ksize throughout (-1: Scharr).
// A lane holds 4 neighbouring pixels of a row as two packed int16 pairs, its neighbours in the wave the pixels left and
// right of them.  Per source row the horizontal pass gives the derivative (hd) and smoothing (hs) rows; the caller keeps the
// last RING of them per channel in registers, and the vertical pass combines the newest ksize.  Device only, registers
// only; every ring slot is a compile-time index.
#pragma once
#include "canny_device.h"

namespace hc {
namespace sep {  // the short helper names stay out of hc: the two users say `using namespace sep`

typedef short i16x2v __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ i16x2v V(u32 v) { return __builtin_bit_cast(i16x2v, v); }
static __device__ __forceinline__ u32 W32(i16x2v v) { return __builtin_bit_cast(u32, v); }
static __device__ __forceinline__ i16x2v splat(int c) { return i16x2v{ (short)c, (short)c }; }
static __device__ __forceinline__ int lo16(u32 v) { return (int)(short)(v & 0xFFFFu); }
static __device__ __forceinline__ int hi16(u32 v) { return (int)v >> 16; }
// (half LH of lo_src, half HH of hi_src) as one int16 pair
template <int LH, int HH>
static __device__ __forceinline__ u32 pick2(u32 lo_src, u32 hi_src)
{
  return __builtin_amdgcn_perm(hi_src, lo_src, (LH ? 0x0302u : 0x0100u) | ((HH ? 0x0706u : 0x0504u) << 16));
}

constexpr int deriv_taps(int kind) { return kind == -1 ? 3 : kind; }
constexpr int smooth_tap(int kind, int t)
{
  constexpr int s3[3] = { 1, 2, 1 }, s5[5] = { 1, 4, 6, 4, 1 }, s7[7] = { 1, 6, 15, 20, 15, 6, 1 }, sc[3] = { 3, 10, 3 };
  return kind == 3 ? s3[t] : kind == 5 ? s5[t] : kind == 7 ? s7[t] : sc[t];
}
constexpr int deriv_tap(int kind, int t)
{
  constexpr int d3[3] = { -1, 0, 1 }, d5[5] = { -1, -2, 0, 2, 1 }, d7[7] = { -1, -4, -5, 0, 5, 4, 1 };
  return kind == 5 ? d5[t] : kind == 7 ? d7[t] : d3[t];
}

// channel ch of the lane's 4 pixels as one dword, replicated at the borders by the caller's byte selector rsel (the few
// lines that make it stay in each kernel: as a function here they changed the prologue of every one of them).  d: the
// group's NC dwords as loaded; of 12 interleaved bytes the channel's (ch, ch + 3, ch + 6, ch + 9) are picked first
template <int NC>
static __device__ __forceinline__ u32 pick_channel(const u32 (&d)[NC], int ch, u32 rsel)
{
  u32 v = d[0];
  if constexpr (NC == 3) {
    const u32 selA = ch == 0 ? 0x0c060300u : ch == 1 ? 0x0c070401u : 0x0c0c0502u;
    const u32 selB = ch == 0 ? 0x05020100u : ch == 1 ? 0x06020100u : 0x07040100u;
    v = __builtin_amdgcn_perm(d[2], __builtin_amdgcn_perm(d[1], d[0], selA), selB);
  }
  return __builtin_amdgcn_perm(0u, v, rsel);
}

// The passes work on one pixel pair h (pixels 2 h, 2 h + 1) and the caller loops over h = 0, 1: with that loop inside
// them the compiler scheduled k_deriv16 differently (66 instead of 96 registers at ksize 7) and measurably slower.
// the pair window of a row: b = the lane's 4 pixels -> P[t + 4] = the pixel pair that starts t columns from the lane's first
struct PairWindow { u32 p[11]; };
static __device__ __forceinline__ PairWindow sep_window(u32 b)
{
  PairWindow w;
  u32 (&P)[11] = w.p;
  P[4] = unpack_lo(b); P[6] = unpack_hi(b);
  P[2] = from_lane_below(P[6]); P[8] = from_lane_above(P[4]);
  P[0] = from_lane_below(P[4]); P[10] = from_lane_above(P[6]);
  P[1] = pair_shift(P[2], P[0]); P[3] = pair_shift(P[4], P[2]); P[5] = pair_shift(P[6], P[4]);
  P[7] = pair_shift(P[8], P[6]); P[9] = pair_shift(P[10], P[8]);
  return w;
}
// horizontal pass: hd / hs of pair h.  Packed int16 for every kind: |hd| <= 255 * (sum of the positive derivative taps)
// and hs <= 255 * (sum of the smoothing taps), at most |hd| <= 2550 and hs <= 16320 (ksize 7)
template <int KIND>
static __device__ __forceinline__ void sep_hpass(const PairWindow &w, int h, u32 &hd1, u32 &hs1)
{
  const u32 (&P)[11] = w.p;
  constexpr int K = deriv_taps(KIND), RAD = K / 2;
  const int c = 4 + 2 * h;
  i16x2v hs = V(P[c]) * splat(smooth_tap(KIND, RAD)), hd = splat(0);
#pragma unroll
  for (int t = 0; t < RAD; ++t) {
    hs += (V(P[c - RAD + t]) + V(P[c + RAD - t])) * splat(smooth_tap(KIND, t));
    hd += (V(P[c + RAD - t]) - V(P[c - RAD + t])) * splat(deriv_tap(KIND, K - 1 - t));
  }
  hs1 = W32(hs);
  hd1 = W32(hd);
}

// vertical pass over the newest K = deriv_taps(KIND) rows of the rings HD / HS [slot][pair], the newest in slot u: dx / dy
// of pair h.  The slot of tap t (t = 0: the oldest row) is (u + RING - (K - 1) + t) % RING.
// Packed int16 for ksize 3, 5 and -1.  The results are at most 255 * (sum of one kind of taps) * (sum of the other's
// positive ones): |dx|, |dy| <= 1020 (ksize 3), 4080 (Scharr), 12240 (ksize 5); partial sums may wrap on the way there
template <int KIND, int RING, int u>
static __device__ __forceinline__ void sep_vpass_pk(const u32 (&HD)[RING][2], const u32 (&HS)[RING][2], int h, u32 &dx, u32 &dy)
{
  constexpr int K = deriv_taps(KIND), RAD = K / 2, OLD = u + RING - (K - 1);
  static_assert(KIND != 7 && RING >= K && u >= 0 && u < RING, "the ring holds the K newest rows");
  i16x2v vx = V(HD[(OLD + RAD) % RING][h]) * splat(smooth_tap(KIND, RAD)), vy = splat(0);
#pragma unroll
  for (int t = 0; t < RAD; ++t) {
    const int so = (OLD + t) % RING, sn = (OLD + K - 1 - t) % RING;  // rows RAD - t above and below the output row
    vx += (V(HD[so][h]) + V(HD[sn][h])) * splat(smooth_tap(KIND, t));
    vy += (V(HS[sn][h]) - V(HS[so][h])) * splat(deriv_tap(KIND, K - 1 - t));
  }
  dx = W32(vx);
  dy = W32(vy);
}
// ksize 7, as one 32-bit value per pixel: symmetric rows first, still packed (sums of two hd and differences of two hs fit
// int16), the products summed in 32 bits: |S| <= 2550 * 64 = 16320 * 10 = 163200, then S / 16 rounded half to even
template <int RING, int u>
static __device__ __forceinline__ void sep_vpass_wide(const u32 (&HD)[RING][2], const u32 (&HS)[RING][2], int h, int &dx0, int &dx1, int &dy0, int &dy1)
{
  constexpr int KIND = 7, K = 7, RAD = 3, OLD = u + RING - (K - 1);
  static_assert(RING >= K && u >= 0 && u < RING, "the ring holds the K newest rows");
  const u32 mid = HD[(OLD + RAD) % RING][h];
  int sx0 = lo16(mid) * smooth_tap(KIND, RAD), sx1 = hi16(mid) * smooth_tap(KIND, RAD), sy0 = 0, sy1 = 0;
#pragma unroll
  for (int t = 0; t < RAD; ++t) {
    const int so = (OLD + t) % RING, sn = (OLD + K - 1 - t) % RING;
    const u32 a = W32(V(HD[so][h]) + V(HD[sn][h]));
    const u32 d = W32(V(HS[sn][h]) - V(HS[so][h]));
    sx0 += lo16(a) * smooth_tap(KIND, t); sx1 += hi16(a) * smooth_tap(KIND, t);
    sy0 += lo16(d) * deriv_tap(KIND, K - 1 - t); sy1 += hi16(d) * deriv_tap(KIND, K - 1 - t);
  }
  auto rnd = [](int s) -> int { return (s + 7 + ((s >> 4) & 1)) >> 4; };  // what cvRound gives for the exact float S / 16
  dx0 = rnd(sx0); dx1 = rnd(sx1);
  dy0 = rnd(sy0); dy1 = rnd(sy1);
}

}  // namespace sep
}  // namespace hc
