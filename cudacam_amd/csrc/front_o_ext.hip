// front_o_ext.hip -- the rest of cv::Canny's surface for Mode O: apertures 5, 7 and -1 (Scharr), and the (dx, dy) overload.
//
// One kernel template, four row sources and a shared back half:
//   SRC 0  u8 rows (1 or 3 interleaved channels) -> the 5x5 Sobel of cv::Canny(img, low, high, 5, L2gradient), separably in
//          packed 16-bit math, spelled out below (every partial and final sum fits int16: |dx|, |dy| <= 12240)
//   SRC 1  int16 dx / dy rows given by the caller (cv::Canny(dx, dy, edges, low, high, L2gradient))
//   SRC 2  u8 rows -> the 7x7 Sobel (scale 1/16) of cv::Canny(img, low, high, 7, L2gradient)
//   SRC 3  u8 rows -> the Scharr derivatives of cv::Canny(img, low, high, -1, L2gradient)
//          SRC 2 and 3 are sep_deriv.h's horizontal and vertical pass at ksize 7 and -1, the arithmetic of k_deriv16
//          (deriv.hip); the taps and the int16 ranges are stated there
//   back   32-bit magnitude (L1 |dx| + |dy| or L2 dx^2 + dy^2, two's complement with wrap-around as canny.cpp's `int`),
//          the 3-channel "first channel with the largest m" select, the integer tangent test (TG22 = 13573), asymmetric
//          non-maximum suppression and the two thresholds -> STRONG / CANDIDATE bit planes that k_hyst finishes.
// Layout as k_front_o (canny_kernels.hip): a wave owns a 248-column strip, lane l the 4 pixels at strip * 248 - 4 + 4 l,
// lanes 0 and 63 are halo (aperture 5 needs 2 Sobel + 1 NMS columns of the 4 a halo lane holds, aperture 7 all of them: 3
// Sobel + 1 NMS); a work item is (frame, strip, chunk of rows) with a warm-up of 3 (SRC 0) / 1 (SRC 1) / 4 (SRC 2) / 2
// (SRC 3) rows; registers only, nothing but the bit planes goes to memory.
// Rings: the source ring holds 6 (SRC 0), 7 (SRC 2) or 3 (SRC 3) rows, the magnitude ring 3, the dx / dy ring 2.  SRC 0, 1
// and 3 unroll 6 steps per loop trip, the common period, so every ring slot is a compile-time register.  A 7-row source
// ring would make that period 42: SRC 2 unrolls the 7 steps of its source ring and advances the two small rings by
// register moves instead (the unrolled body renames them: the moves that remain sit at the loop's back edge).
#include "sep_deriv.h"

namespace hc {

namespace {

using namespace sep;

// the u8 sources' cv ksize.  0 -> 5 only documents the map: SRC 0 spells its passes out and never asks (static_assert below)
constexpr int src_kind(int src) { return src == 0 ? 5 : src == 2 ? 7 : -1; }

// TAB (SRC 0 and 1 only): per-frame thresholds from f.frame_thr (as k_front_o: the launcher picks the instantiation)
template <int SRC, bool L2, int NC, bool TAB = false>
__global__ __launch_bounds__(256) void k_front_o_ext(const FrontExtParams e)
{
  constexpr bool U8 = SRC != 1;                            // u8 rows: SRC 0, 2, 3
  constexpr int RING = SRC == 2 ? 7 : SRC == 3 ? 3 : 6;    // source rows kept
  constexpr int PERIOD = SRC == 2 ? 7 : 6;                 // steps per loop trip
  constexpr bool MOVE = SRC == 2;                          // the magnitude and dx / dy rings advance by register moves
  const FrontParams &p = e.f;
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const int item = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + wib);
  if (item >= p.total_items) return;
  const int chunk = item % p.nchunks;
  const int strip = (item / p.nchunks) % p.nstrips;
  const int frame = item / (p.nchunks * p.nstrips);
  const int W = p.W, H = p.H, CH = p.chunk_rows;
  const int r0 = chunk * CH, rend = min(r0 + CH, H);
  const int c0 = strip * STRIP_W - STRIP_HALO + lane * PX_PER_LANE;
  constexpr int LAG = SRC == 0 ? 2 : SRC == 2 ? 3 : SRC == 3 ? 1 : 0;  // gradient row = source row - LAG
  const int rlast = min(H - 1, rend + LAG);    // last source row this item needs

  bool cin[4];  // the lane's columns inside the image (m = 0 outside)
#pragma unroll
  for (int q = 0; q < 4; ++q) cin[q] = c0 + q >= 0 && c0 + q < W;
  u32 oknib = 0;
  if (lane >= 1 && lane <= 62)
#pragma unroll
    for (int q = 0; q < 4; ++q) oknib |= cin[q] ? (0x101u << q) : 0u;

  // ---- SRC 0, 2, 3: u8 rows, BORDER_REPLICATE by clamping (rows) and a per-lane byte selector (columns), as k_front_o ----
  u32 rsel = 0;
  int ld_col = 0;
  if constexpr (U8) {
    const int cl0 = min(max(c0, 0), W - 1);
    ld_col = cl0 & ~3;
#pragma unroll
    for (int k = 0; k < 4; ++k) rsel |= (u32)(min(max(c0 + k, 0), W - 1) - ld_col) << (8 * k);
  }
  const uint8_t *fbase = p.in + (size_t)frame * p.in_frame_stride;   // SRC 1: dx
  const uint8_t *fbase_y = e.dy + (size_t)frame * p.in_frame_stride; // SRC 1: dy (same pitch / frame stride)
  const int ne = NC * W, e0 = NC * c0;  // SRC 1: int16 elements per row, the lane's first element (even)
  constexpr int ND = U8 ? NC : 4 * NC;  // dwords per lane and row: 4 px x NC bytes, or 2 planes x 4 px x NC int16
  struct Raw { u32 d[ND]; };
  // one int16 pair (elements ei, ei + 1) of a row; reads nothing outside [row start, row start + 2 * ne)
  auto ld_pair = [&](const uint8_t *rp, bool al, int ei) -> u32 {
    const unsigned short *h = reinterpret_cast<const unsigned short *>(rp) + ei;
    if (ei >= 0 && ei + 1 < ne) {
      if (al) return *reinterpret_cast<const u32 *>(h);
      return (u32)h[0] | ((u32)h[1] << 16);
    }
    return (ei >= 0 && ei < ne) ? (u32)h[0] : 0u;
  };
  auto load_row = [&](int row) -> Raw {
    const int rr = min(max(row, 0), rlast);
    Raw r;
    if constexpr (U8) {
      const u32 *q = reinterpret_cast<const u32 *>(fbase + (size_t)rr * p.in_pitch + (size_t)(NC * ld_col));
#pragma unroll
      for (int i = 0; i < NC; ++i) r.d[i] = q[i];
    } else {
      const uint8_t *rx = fbase + (size_t)rr * p.in_pitch, *ry = fbase_y + (size_t)rr * p.in_pitch;
      const bool ax = ((uintptr_t)rx & 3u) == 0, ay = ((uintptr_t)ry & 3u) == 0;  // wave-uniform
#pragma unroll
      for (int j = 0; j < 2 * NC; ++j) {
        r.d[j] = ld_pair(rx, ax, e0 + 2 * j);
        r.d[2 * NC + j] = ld_pair(ry, ay, e0 + 2 * j);
      }
    }
    return r;
  };
  // u8 rows: per channel, the horizontal derivative / smoothing rows of the last RING source rows, packed pairs [ring][pair]
  constexpr int NR = U8 ? NC : 1;
  u32 HD[NR][RING][2], HS[NR][RING][2];
#pragma unroll
  for (int ch = 0; ch < NR; ++ch)
#pragma unroll
    for (int a = 0; a < RING; ++a) HD[ch][a][0] = HD[ch][a][1] = HS[ch][a][0] = HS[ch][a][1] = 0;
  int Mr[3][6];      // magnitude rows: [ring][0] = left neighbour, [1..4] = own 4 px, [5] = right neighbour
  int Xr[2][4], Yr[2][4];  // dx / dy of the two newest gradient rows
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) Mr[a][b] = 0;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) Xr[a][b] = Yr[a][b] = 0;

  const size_t plane_off = (size_t)frame * H * p.RD * 4;
  uint8_t *splane = reinterpret_cast<uint8_t *>(p.sbits) + plane_off;
  uint8_t *cplane = reinterpret_cast<uint8_t *>(p.cbits) + plane_off;
  const bool store_lane = (lane & 1) && lane < 63;
  const size_t st_off = (size_t)(strip * 31 + (lane >> 1));
  const size_t plane_pitch = (size_t)p.RD * 4u;
  u32 low_u = p.a_lo[0], high_u = p.a_hi[0];
  if constexpr (TAB) frame_thresholds(p.frame_thr, frame, L2, low_u, high_u);  // ... or the frame's own
  const int low = (int)low_u, high = (int)high_u;

  // one step: source row k arrives -> gradient row g = k - LAG -> NMS / threshold row g - 1
  auto step = [&](auto uc, int k, const Raw &raw) {
    constexpr int u = decltype(uc)::value;
    constexpr int rn = MOVE ? 1 : u % 2, rp = MOVE ? 0 : (u + 1) % 2;
    constexpr int sN = MOVE ? 2 : u % 3, sC = MOVE ? 1 : (u + 2) % 3, sU = MOVE ? 0 : (u + 1) % 3;
    const int g = k - LAG;
    if constexpr (MOVE) {
#pragma unroll
      for (int b = 0; b < 6; ++b) { Mr[0][b] = Mr[1][b]; Mr[1][b] = Mr[2][b]; }
#pragma unroll
      for (int q = 0; q < 4; ++q) { Xr[0][q] = Xr[1][q]; Yr[0][q] = Yr[1][q]; }
    }
    int X[4], Y[4], M[4];
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
      int x[4], y[4];
      if constexpr (SRC == 0) {
        // spelled out: through sep_deriv.h's loops at ksize 5 in a ring of 6 the fused aperture-5 runs measured 0.6-0.9 % slower
        // horizontal pass on the new row: hd = [-1 -2 0 2 1], hs = [1 4 6 4 1] (pairs of int16, wrapping sums that end in range)
        const u32 b = pick_channel(raw.d, ch, rsel);
        const u32 A = unpack_lo(b), B = unpack_hi(b);           // (x0, x1), (x2, x3)
        const u32 Bl = from_lane_below(B), Ar = from_lane_above(A);  // (x-2, x-1), (x4, x5)
        const u32 m1 = pair_shift(A, Bl), p1 = pair_shift(B, A), p3 = pair_shift(Ar, B);  // (x-1, x0), (x1, x2), (x3, x4)
        const i16x2v two = { 2, 2 }, four = { 4, 4 }, six = { 6, 6 };
        HD[ch][u][0] = W32(V(B) - V(Bl) + two * (V(p1) - V(m1)));
        HS[ch][u][0] = W32(V(Bl) + V(B) + four * (V(m1) + V(p1)) + six * V(A));
        HD[ch][u][1] = W32(V(Ar) - V(A) + two * (V(p3) - V(p1)));
        HS[ch][u][1] = W32(V(A) + V(Ar) + four * (V(p1) + V(p3)) + six * V(B));
        // vertical pass over source rows k-4 .. k: dx = [1 4 6 4 1] on hd, dy = [-1 -2 0 2 1] on hs
        constexpr int s0 = (u + 2) % 6, s1 = (u + 3) % 6, s2 = (u + 4) % 6, s3 = (u + 5) % 6, s4 = u;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const u32 dxp = W32(V(HD[ch][s0][h]) + V(HD[ch][s4][h]) + four * (V(HD[ch][s1][h]) + V(HD[ch][s3][h])) + six * V(HD[ch][s2][h]));
          const u32 dyp = W32(V(HS[ch][s4][h]) - V(HS[ch][s0][h]) + two * (V(HS[ch][s3][h]) - V(HS[ch][s1][h])));
          x[2 * h] = lo16(dxp); x[2 * h + 1] = hi16(dxp);
          y[2 * h] = lo16(dyp); y[2 * h + 1] = hi16(dyp);
        }
      } else if constexpr (U8) {
        // sep_deriv.h's two passes; the vertical one over the newest deriv_taps(KIND) rows of the ring
        static_assert(SRC == 2 || SRC == 3, "the shared passes serve aperture 7 and Scharr");
        constexpr int KIND = src_kind(SRC), us = u % RING;
        const PairWindow P = sep_window(pick_channel(raw.d, ch, rsel));
#pragma unroll
        for (int h = 0; h < 2; ++h) sep_hpass<KIND>(P, h, HD[ch][us][h], HS[ch][us][h]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if constexpr (KIND == 7) sep_vpass_wide<RING, us>(HD[ch], HS[ch], h, x[2 * h], x[2 * h + 1], y[2 * h], y[2 * h + 1]);
          else {
            u32 px, py;
            sep_vpass_pk<KIND, RING, us>(HD[ch], HS[ch], h, px, py);
            x[2 * h] = lo16(px); x[2 * h + 1] = hi16(px);
            y[2 * h] = lo16(py); y[2 * h + 1] = hi16(py);
          }
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ei = NC * q + ch;
          const u32 wx = raw.d[ei >> 1], wy = raw.d[2 * NC + (ei >> 1)];
          x[q] = (ei & 1) ? hi16(wx) : lo16(wx);
          y[q] = (ei & 1) ? hi16(wy) : lo16(wy);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // canny.cpp computes in int: the L2 sum wraps (to INT_MIN for dx = dy = -32768 only)
        const int m = L2 ? (int)((u32)(x[q] * x[q]) + (u32)(y[q] * y[q])) : abs(x[q]) + abs(y[q]);
        if (ch == 0 || m > M[q]) {  // first channel with the largest magnitude
          M[q] = m; X[q] = x[q]; Y[q] = y[q];
        }
      }
    }
    const bool rowbad = g < 0 || g >= H;  // wave-uniform: magnitude outside the image is 0
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      Mr[sN][1 + q] = (rowbad || !cin[q]) ? 0 : M[q];
      Xr[rn][q] = X[q];
      Yr[rn][q] = Y[q];
    }
    Mr[sN][0] = (int)from_lane_below((u32)Mr[sN][4]);
    Mr[sN][5] = (int)from_lane_above((u32)Mr[sN][1]);

    const int c = g - 1;
    if (c >= r0 && c < rend) {
      u32 nib = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = Mr[sC][1 + q];
        const int xs = Xr[rp][q], ys = Yr[rp][q];
        // tangent test in int, as canny.cpp: tg67x wraps for |dx| >= 27146 (then y > tg67x: the vertical branch)
        const u32 ax = (u32)abs(xs), ay = (u32)abs(ys);
        const int y15 = (int)(ay << 15), tg22x = (int)(ax * 13573u), tg67x = (int)(ax * 13573u + (ax << 16));
        const bool kh = m > Mr[sC][q] && m >= Mr[sC][2 + q];       // left, right
        const bool kv = m > Mr[sU][1 + q] && m >= Mr[sN][1 + q];   // up, down
        const bool kp = m > Mr[sU][q] && m > Mr[sN][2 + q];        // s = +1: up-left, down-right
        const bool kn = m > Mr[sU][2 + q] && m > Mr[sN][q];        // s = -1: up-right, down-left
        const bool keep = m > low && (y15 < tg22x ? kh : y15 > tg67x ? kv : ((xs ^ ys) < 0 ? kn : kp));
        nib |= (keep ? (0x100u << q) : 0u) | ((keep && m > high) ? (1u << q) : 0u);
      }
      nib &= oknib;
      const u32 w = nib | (from_lane_above(nib) << 4);
      if (store_lane) {
        const size_t roff = (size_t)c * plane_pitch + st_off;
        splane[roff] = (uint8_t)w;
        cplane[roff] = (uint8_t)(w >> 8);
      }
    }
  };

  // source rows r0 - LAG - 1 .. rend + LAG, PERIOD steps per loop trip (the ring period); a row is requested PERIOD steps
  // before it is used (as k_front_o)
  const int k0 = r0 - LAG - 1, kend = rend + LAG + 1;
  Raw bn[PERIOD];
#pragma unroll
  for (int j = 0; j < PERIOD; ++j) bn[j] = load_row(k0 + j);
  auto advance = [&](auto uc, int k) {
    constexpr int j = decltype(uc)::value;
    const Raw b = bn[j];
    bn[j] = load_row(k + PERIOD);
    step(uc, k, b);
  };
#pragma nounroll
  for (int k = k0; k < kend; k += PERIOD) {
    advance(std::integral_constant<int, 0>{}, k + 0);
    advance(std::integral_constant<int, 1>{}, k + 1);
    advance(std::integral_constant<int, 2>{}, k + 2);
    advance(std::integral_constant<int, 3>{}, k + 3);
    advance(std::integral_constant<int, 4>{}, k + 4);
    advance(std::integral_constant<int, 5>{}, k + 5);
    if constexpr (PERIOD == 7) advance(std::integral_constant<int, 6>{}, k + 6);
  }
}

template <int SRC>
hipError_t launch_src(const FrontExtParams &e, const dim3 grid, const dim3 block, hipStream_t s)
{
  const bool three = SRC != 1 ? e.f.bgr != 0 : e.channels == 3;
  // a per-frame table applies to aperture 5 and given gradients (hc_canny_device's fused sources take the call's pair)
  auto go = [&](auto l2, auto nc) {
    constexpr bool L2 = decltype(l2)::value;
    constexpr int NC = decltype(nc)::value;
    if constexpr (SRC <= 1) {
      if (e.f.frame_thr) { hipLaunchKernelGGL((k_front_o_ext<SRC, L2, NC, true>), grid, block, 0, s, e); return; }
    }
    hipLaunchKernelGGL((k_front_o_ext<SRC, L2, NC, false>), grid, block, 0, s, e);
  };
  using std::integral_constant;
  if (SRC > 1 && e.f.frame_thr) return hipErrorInvalidValue;
  if (three) {
    if (e.f.l2gradient) go(integral_constant<bool, true>{}, integral_constant<int, 3>{});
    else go(integral_constant<bool, false>{}, integral_constant<int, 3>{});
  } else {
    if (e.f.l2gradient) go(integral_constant<bool, true>{}, integral_constant<int, 1>{});
    else go(integral_constant<bool, false>{}, integral_constant<int, 1>{});
  }
  return hipGetLastError();
}

}  // namespace

// gradients == 0: u8 frames at f.in (f.bgr: 3 interleaved channels; rows hold whole 4-pixel groups, pitch >= C * round_up(W, 4),
// multiple of 4), e.aperture 5, 7 or -1 picks the source; gradients != 0: int16 dx at f.in, dy at e.dy, `channels` interleaved, even pitch >= 2 * channels * W
hipError_t launch_front_o_ext(const FrontExtParams &e, hipStream_t s)
{
  const FrontParams &p = e.f;
  if (p.chunk_rows < 1 || p.W < 1 || p.H < 1) return hipErrorInvalidValue;
  const dim3 grid((p.total_items + 3) / 4), block(256);
  if (e.gradients) {
    if (!e.dy || (e.channels != 1 && e.channels != 3) || ((p.in_pitch | p.in_frame_stride) & 1u)
        || p.in_pitch < (size_t)2 * e.channels * p.W)
      return hipErrorInvalidValue;
    return launch_src<1>(e, grid, block, s);
  }
  if ((p.in_pitch & 3u) || p.in_pitch < (size_t)(p.bgr ? 3 : 1) * (((size_t)p.W + 3) / 4 * 4)) return hipErrorInvalidValue;
  switch (e.aperture) {
  case 5: return launch_src<0>(e, grid, block, s);
  case 7: return launch_src<2>(e, grid, block, s);
  case -1: return launch_src<3>(e, grid, block, s);
  default: return hipErrorInvalidValue;
  }
}

}  // namespace hc
