// canny_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of hipcanny beside the two big ones.
//
// What the reference does in 9+k launches over 25 B/px of intermediates (src/cvp/cannyEdgeD.cu,
// launch sites src/cvp/cannyEdgeH.cu:214-338) is done by k_front8 (front8.hip: the whole front path, one kernel) and
// k_hyst (hyst.hip: edge hysteresis on the bit planes, 0/255 u8 edge map written by the same kernel).  Here:
//   k_selftest  the cross-lane and packed primitives of canny_device.h, checked on the device (hc_selftest)
//   k_front_o   the 4-px cv::Canny ("Mode O") front kernel (3-channel sources; one-channel sources: k_front8o, front8.hip)
//   k_copy_rows pitched copies between caller buffers the kernels cannot use in place and the context's own
// (the round-1 front kernels of Mode R -- k_front, k_blur + k_nms -- live in legacy_front.hip, outside the product library)
// plus the plain per-stage kernels behind the finalStage taps.
// MFMA is deliberately not used: there is no dense contraction (an f32 MFMA would reproduce the
// Gaussian's fmaf chain bit for bit, but as a banded 36x32 Toeplitz product it wastes 31/36 of its
// multiplies and runs at the f32 vector rate -- 4-7x slower than the packed integer form below).
//
// Numerical contract ("Mode R"): identical to the reference kernels, including the
// float Gaussian chain (via the exact integer shortcut explained in front8.hip), the u8 wrap of gradients
// >= 256 and the non-strict NMS.
#include "canny_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace hc {

// The reference uploads its coefficient table to __constant__ GK[5][5] (cannyEdgeD.cu:11, cannyEdgeH.cu:372-380); here the
// 25 values are literals of the instruction stream (as __constant__ loads they pinned 25 SGPRs across the hot loops), so
// the host's table -- computed the reference's way at hc_create -- is only CHECKED against them.
hipError_t check_gauss_coeffs(const float gk[25])
{
  return memcmp(gk, GKC.v, sizeof(GKC.v)) == 0 ? hipSuccess : hipErrorInvalidValue;
}

// =================================================================================================
// Self-test of the primitives above (hc_selftest): catches a wrong DPP direction or perm selector.
// =================================================================================================
__global__ void k_selftest(u32 *res)
{
  const u32 lane = threadIdx.x & 63;
  u32 bad = 0;
  bad |= (from_lane_below(lane + 100) != (lane ? lane + 99 : 0)) ? 1u : 0u;
  bad |= (from_lane_above(lane + 100) != (lane < 63 ? lane + 101 : 0)) ? 2u : 0u;
  const u32 x = 0x44332211u + lane;
  bad |= (unpack_lo(x) != ((x & 0xFF) | (((x >> 8) & 0xFF) << 16))) ? 4u : 0u;
  bad |= (unpack_hi(x) != (((x >> 16) & 0xFF) | ((x >> 24) << 16))) ? 8u : 0u;
  bad |= (pair_shift(0xAAAA1111u + lane, 0x2222BBBBu) != (((0xAAAA1111u + lane) << 16) | 0x2222u)) ? 16u : 0u;
  const u32 p0 = 0x00050003u, p1 = 0x00090007u;
  bad |= (__builtin_amdgcn_perm(p1, p0, 0x06040200u) != 0x09070503u) ? 32u : 0u;
  bad |= (__builtin_amdgcn_perm(0x00BB00AAu, 0x00220011u, 0x05040100u) != 0x00AA0011u) ? 64u : 0u;
  bad |= (__builtin_amdgcn_perm(0x00BB00AAu, 0x00220011u, 0x07060302u) != 0x00BB0022u) ? 128u : 0u;
  bad |= (__builtin_amdgcn_udot2(U(0x9E61u | (40545u << 16)), U(0x0000CE17u), 0u, false) != 0x9E61u * 52759u) ? 256u : 0u;
  bad |= (__builtin_amdgcn_sdot2(I(0xFC04u | (1020u << 16)), I(0xFC04u | (1020u << 16)), 0, false) != 2 * 1020 * 1020) ? 512u : 0u;
  const u64 m = __ballot(lane & 1);
  bad |= (m != 0xAAAAAAAAAAAAAAAAull) ? 1024u : 0u;
  bad |= (mbcnt64(m) != lane / 2) ? 2048u : 0u;
  bad |= (shift_in(lane, m) != 2 * lane + (lane & 1)) ? 4096u : 0u;
  {
    const int xl = (int)lane - 32, xh = 1000 - 3 * (int)lane;            // packed i16 pair (xl, xh)
    const u32 pk = ((u32)xl & 0xFFFFu) | ((u32)xh << 16);
    bad |= (mul16<0, 0>(pk, pk) != xl * xl) ? 8192u : 0u;
    bad |= (mul16<1, 1>(pk, pk) != xh * xh) ? 8192u : 0u;
    bad |= (mad16<0, 1>(pk, pk, 7) != xl * xh + 7) ? 8192u : 0u;
    bad |= (mad16<1, 0>(pk, pk, -5) != xh * xl - 5) ? 8192u : 0u;
  }
  if (bad) atomicOr(res, bad);
}

hipError_t launch_selftest(u32 *d_result, hipStream_t s)
{
  hipLaunchKernelGGL(k_selftest, dim3(2), dim3(128), 0, s, d_result);
  return hipGetLastError();
}

// =================================================================================================
// k_front_o: "Mode O" -- cv::Canny(src 8UC1, low, high, apertureSize 3, L2gradient) semantics
// =================================================================================================
// OpenCV 4.x modules/imgproc/src/canny.cpp (the parity tests check it against a CPU restatement): no blur,
// Sobel 3x3 on the source with BORDER_REPLICATE, magnitude m = |dx|+|dy| (or dx^2+dy^2 with L2gradient; 0
// outside the image), pixels with m <= low are dropped, direction by the integer tangent test
// (TG22 = 13573, shift 15), asymmetric non-maximum suppression (m > first neighbour, m >= second on the
// axes; strict on both diagonal neighbours), m > high seeds.  Same strip / lane / DPP layout and the same
// bit-plane output as k_nms, so k_hyst finishes the job.  One pass, registers only (no LDS): a work item is
// (frame, strip, chunk of p.chunk_rows rows) with a 4-row warm-up.
// NC: channels of the (interleaved) source.  cv::Canny on a 3-channel image computes the Sobel derivatives of every
// channel and keeps, per pixel, those of the channel with the largest magnitude -- the first one on ties (canny.cpp).
// TAB: the thresholds come from the per-frame table p.frame_thr (non-null) instead of p.a_lo[0] / p.a_hi[0]; the launcher picks
// the instantiation, so runs without a table execute the code they always did
template <bool L2, int NC, bool TAB = false>
__global__ __launch_bounds__(256) void k_front_o(const FrontParams p)
{
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

  // BORDER_REPLICATE along the row: the 4 columns of this lane, clamped into the image, always lie in
  // one aligned dword; a per-lane byte selector arranges (and repeats) them
  u32 cmask = 0, rsel = 0;
  const int cl0 = min(max(c0, 0), W - 1);
  const int ld_col = cl0 & ~3;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in = (c0 + k >= 0) && (c0 + k < W);
    cmask |= in ? (0xFFu << (8 * k)) : 0u;
    const int cc = min(max(c0 + k, 0), W - 1);
    rsel |= (u32)(cc - ld_col) << (8 * k);  // 0..3: byte of the loaded dword (cc - ld_col < 4 by construction)
  }
  const u32 pm0 = __builtin_amdgcn_perm(0u, cmask, 0x01010000u), pm1 = __builtin_amdgcn_perm(0u, cmask, 0x03030202u);
  const u32 oknib1 = (lane >= 1 && lane <= 62) ? ((cmask & 1u) | ((cmask >> 7) & 2u) | ((cmask >> 14) & 4u) | ((cmask >> 21) & 8u)) : 0u;
  const u32 oknib = oknib1 | (oknib1 << 8);
  const uint8_t *fbase = p.in + (size_t)frame * p.in_frame_stride;  // wave-uniform
  const u32 in_pitch32 = (u32)p.in_pitch;                            // launch_front_o checks H * pitch < 2^32
  const u32 ld_off = (u32)(NC * ld_col);
  const int rlast = min(H - 1, rend + 1);  // last source row this run needs
  struct RawO { u32 d[NC]; };  // the lane's 4 pixels as loaded: 4 bytes, or 12 interleaved ones
  auto load_row = [&](int row) -> RawO {  // BORDER_REPLICATE along the column: clamp the row; the raw dwords (see use_row)
    const int rr = min(max(row, 0), rlast);
    u32 roff;
    asm("s_mul_i32 %0, %1, %2" : "=s"(roff) : "s"(rr), "s"(in_pitch32));
    u32 o = ld_off;
    asm volatile("" : "+v"(o));  // scalar row base + 32-bit lane offset
    const u32 *q = reinterpret_cast<const u32 *>(fbase + roff + o);
    RawO r;
#pragma unroll
    for (int i = 0; i < NC; ++i) r.d[i] = q[i];
    return r;
  };
  // BORDER_REPLICATE along the row: the byte selector, applied when the row is consumed -- applied at the load it
  // made the wave wait for each request at once.  3-channel data: channel ch of the 4 pixels is picked out of the
  // 12 interleaved bytes first (bytes ch, ch+3, ch+6, ch+9).
  auto use_row = [&](const RawO &raw, int ch) -> u32 {
    u32 v = raw.d[0];
    if constexpr (NC == 3) {
      const u32 selA = ch == 0 ? 0x0c060300u : ch == 1 ? 0x0c070401u : 0x0c0c0502u;
      const u32 selB = ch == 0 ? 0x05020100u : ch == 1 ? 0x06020100u : 0x07040100u;
      v = __builtin_amdgcn_perm(raw.d[NC > 2 ? 2 : 0], __builtin_amdgcn_perm(raw.d[NC > 1 ? 1 : 0], raw.d[0], selA), selB);
    }
    return __builtin_amdgcn_perm(0u, v, rsel);
  };

  u32 dr[NC][2][2], sr[NC][2][2];  // per channel: d = x[+1]-x[-1] and s = x[-1]+2x[0]+x[+1] of the two previous rows, [ring][pair]
  u32 Mr[3][6];            // magnitude rows: [ring][0]=left neighbour, [1..4]=own 4 px, [5]=right neighbour
  u32 Xr[2][2], Yr[2][2];  // packed dx / dy pairs of the two newest gradient rows
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      Xr[a][b] = Yr[a][b] = 0;
#pragma unroll
      for (int ch = 0; ch < NC; ++ch) dr[ch][a][b] = sr[ch][a][b] = 0;
    }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) Mr[a][b] = 0;
  const size_t plane_off = (size_t)frame * H * p.RD * 4;
  uint8_t *splane = reinterpret_cast<uint8_t *>(p.sbits) + plane_off;
  uint8_t *cplane = reinterpret_cast<uint8_t *>(p.cbits) + plane_off;
  const bool store_lane = (lane & 1) && lane < 63;
  const u32 st_off = (u32)(strip * 31 + (lane >> 1));
  const u32 plane_pitch = (u32)p.RD * 4u;
  u32 low = p.a_lo[0], high = p.a_hi[0];  // Mode O: plain thresholds on m
  if constexpr (TAB) frame_thresholds(p.frame_thr, frame, L2, low, high);  // ... or the frame's own
  const u32 k_tg22 = 13573u, k_m32768 = 0x8000u;  // 16-bit multiplier operands (low halves): TG22 and -2^15

  // one step: source row k arrives -> gradient row k-1 -> NMS / threshold row k-2
  auto step = [&](auto uc, int k, const RawO &raw) {
    constexpr int u = decltype(uc)::value;
    constexpr int rn = u % 2, rp = (u + 1) % 2;
    constexpr int sN = u % 3, sC = (u + 2) % 3, sU = (u + 1) % 3;
    const int i = k - 1;  // gradient row from source rows k-2 (ring rn), k-1 (ring rp), k (new)
    const bool rowbad = i < 0 || i >= H;  // magnitude outside the image is 0
    u32 Xv[2] = { 0, 0 }, Yv[2] = { 0, 0 };   // dx / dy of the channel kept so far, [pair]
    u32 Mp[2] = { 0, 0 };                     // L1: its packed magnitudes
    u32 M4[4] = { 0, 0, 0, 0 };               // L2: its magnitudes, one per pixel
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
      const u32 b = use_row(raw, ch);
      const u32 A = unpack_lo(b), B = unpack_hi(b);
      const u32 Bl = from_lane_below(B), Ar = from_lane_above(A);
      const u32 m1 = pair_shift(A, Bl), p1 = pair_shift(B, A), p3 = pair_shift(Ar, B);
      u32 dk[2], sk[2];
      dk[0] = R(I(p1) - I(m1));
      sk[0] = pk_mad2(A, m1 + p1);
      dk[1] = R(I(p3) - I(p1));
      sk[1] = pk_mad2(B, p1 + p3);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const u32 X = pk_mad2(dr[ch][rp][h], R(I(dr[ch][rn][h]) + I(dk[h]))) & (h == 0 ? pm0 : pm1);  // dx = right - left, smoothed 1-2-1 down the rows
        const u32 Y = R(I(sk[h]) - I(sr[ch][rn][h])) & (h == 0 ? pm0 : pm1);                          // dy = bottom - top
        dr[ch][rn][h] = dk[h];
        sr[ch][rn][h] = sk[h];
        if (L2) {
          const u32 ma = (u32)mad16<0, 0>(X, X, mul16<0, 0>(Y, Y)), mb = (u32)mad16<1, 1>(X, X, mul16<1, 1>(Y, Y));
          if (ch == 0) { Xv[h] = X; Yv[h] = Y; M4[2 * h] = ma; M4[2 * h + 1] = mb; }
          else {  // strictly larger: ties keep the earlier channel
            const bool ta = ma > M4[2 * h], tb = mb > M4[2 * h + 1];
            const u32 msk = (ta ? 0x0000FFFFu : 0u) | (tb ? 0xFFFF0000u : 0u);
            Xv[h] = (X & msk) | (Xv[h] & ~msk);
            Yv[h] = (Y & msk) | (Yv[h] & ~msk);
            M4[2 * h] = ta ? ma : M4[2 * h];
            M4[2 * h + 1] = tb ? mb : M4[2 * h + 1];
          }
        } else {  // |dx| + |dy| <= 2040 per half: packed
          const u32 mp = R(__builtin_elementwise_max(I(X), -I(X))) + R(__builtin_elementwise_max(I(Y), -I(Y)));
          if (ch == 0) { Xv[h] = X; Yv[h] = Y; Mp[h] = mp; }
          else {
            // per half: 0xFFFF where this channel's magnitude is strictly larger (saturating difference, then 0 - min(d, 1))
            const u16x2 dif = __builtin_elementwise_sub_sat(U(mp), U(Mp[h]));
            const u16x2 one = { 1, 1 }, zero = { 0, 0 };
            const u32 msk = R((u16x2)(zero - __builtin_elementwise_min(dif, one)));
            Xv[h] = (X & msk) | (Xv[h] & ~msk);
            Yv[h] = (Y & msk) | (Yv[h] & ~msk);
            Mp[h] = (mp & msk) | (Mp[h] & ~msk);
          }
        }
      }
    }
    if (rowbad) {  // wave-uniform, two rows per frame
      asm volatile("" ::: "memory");  // keeps this one branch instead of per-row selects
      Xv[0] = Xv[1] = Yv[0] = Yv[1] = 0;
      Mp[0] = Mp[1] = 0;
      M4[0] = M4[1] = M4[2] = M4[3] = 0;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      Xr[rn][h] = Xv[h];
      Yr[rn][h] = Yv[h];
      if (L2) {
        Mr[sN][1 + 2 * h] = M4[2 * h];
        Mr[sN][2 + 2 * h] = M4[2 * h + 1];
      } else {
        Mr[sN][1 + 2 * h] = Mp[h] & 0xFFFFu;
        Mr[sN][2 + 2 * h] = Mp[h] >> 16;
      }
    }
    Mr[sN][0] = from_lane_below(Mr[sN][4]);
    Mr[sN][5] = from_lane_above(Mr[sN][1]);

    const int c = k - 2;
    if (c >= r0 && c < rend) {
      u32 nib = 0;
      u64 cl[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) cl[q] = __ballot(Mr[sC][1 + q] > low);
      if ((cl[0] | cl[1] | cl[2] | cl[3]) != 0) {  // rows without a candidate skip direction + NMS
        u32 nibS = 0, nibC = 0;
        auto slot = [&](auto hc, auto ec, u32 aX, u32 aY, u32 X, u32 Y) {
          constexpr int h = decltype(hc)::value, e = decltype(ec)::value, q = 2 * h + e;
          u64 mS = 0, mC = 0;
          if (cl[q] != 0) {
            const u32 m = Mr[sC][1 + q];
            // tangent test on x = |dx|, y = |dy|: horizontal if y*2^15 < x*TG22, vertical if y*2^15 > x*(TG22 + 2^16)
            const int E = mad16<e, 0>(aY, k_m32768, mul16<e, 0>(aX, k_tg22));  // x*TG22 - y*2^15
            const int x16 = (int)(e ? (aX & 0xFFFF0000u) : (aX << 16));          // x * 2^16
            const u64 hz = __ballot(E > 0), vt = __ballot(E + x16 < 0);
            const u64 dneg = __ballot(mul16<e, e>(X, Y) < 0);  // sign(dx) != sign(dy) (both non-zero on a diagonal)
            const u64 kh = __ballot(m > Mr[sC][q]) & __ballot(m >= Mr[sC][2 + q]);       // left, right
            const u64 kv = __ballot(m > Mr[sU][1 + q]) & __ballot(m >= Mr[sN][1 + q]);   // up, down
            const u64 kp = __ballot(m > Mr[sU][q]) & __ballot(m > Mr[sN][2 + q]);        // s = +1: up-left, down-right
            const u64 kn = __ballot(m > Mr[sU][2 + q]) & __ballot(m > Mr[sN][q]);        // s = -1: up-right, down-left
            const u64 dg = ~hz & ~vt;
            const u64 keep = (hz & kh) | (~hz & vt & kv) | (dg & ~dneg & kp) | (dg & dneg & kn);
            mS = __ballot(m > high) & keep;
            mC = cl[q] & keep;
          }
          nibS = shift_in(nibS, mS);
          nibC = shift_in(nibC, mC);
        };
        auto pair = [&](auto hc) {
          constexpr int h = decltype(hc)::value;
          const u32 X = Xr[rp][h], Y = Yr[rp][h];
          const u32 aX = R(__builtin_elementwise_max(I(X), -I(X))), aY = R(__builtin_elementwise_max(I(Y), -I(Y)));
          slot(hc, std::integral_constant<int, 1>{}, aX, aY, X, Y);
          slot(hc, std::integral_constant<int, 0>{}, aX, aY, X, Y);
        };
        pair(std::integral_constant<int, 1>{});
        pair(std::integral_constant<int, 0>{});
        nib = (nibS | (nibC << 8)) & oknib;
      }
      if (p.prov_out && lane >= 1 && lane <= 62 && c0 < W) {  // provisional 0/255 map (strong bits); W % 4 == 0 here
        u32 po;
        asm("s_mul_i32 %0, %1, %2" : "=s"(po) : "s"(c), "s"(p.prov_pitch));
        u32 o = (u32)(strip * STRIP_W + 4 * (lane - 1));
        asm volatile("" : "+v"(o));
        *reinterpret_cast<u32 *>(p.prov_out + (size_t)frame * p.prov_fs + po + o) = nibble_to_bytes(nib & 0xFu);
      }
      const u32 w = nib | (from_lane_above(nib) << 4);
      if (store_lane) {
        u32 roff;
        asm("s_mul_i32 %0, %1, %2" : "=s"(roff) : "s"(c), "s"(plane_pitch));
        u32 so = st_off;
        asm volatile("" : "+v"(so));
        (splane + roff)[so] = (uint8_t)w;
        (cplane + roff)[so] = (uint8_t)(w >> 8);
      }
    }
  };

  // source rows r0-2 .. rend+1, six steps per loop trip (the ring period); a row is requested six steps before it is
  // used and its register refilled at once (unconditional loads: a step waits for the oldest of six, see k_nms)
  const int k0 = r0 - 2, kend = rend + 2;
  RawO bn[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) bn[j] = load_row(k0 + j);
  auto advance = [&](auto uc, int k) {
    constexpr int j = decltype(uc)::value;
    const RawO b = bn[j];
    bn[j] = load_row(k + 6);
    step(uc, k, b);
  };
#pragma nounroll
  for (int k = k0; k < kend; k += 6) {
    advance(std::integral_constant<int, 0>{}, k + 0);
    advance(std::integral_constant<int, 1>{}, k + 1);
    advance(std::integral_constant<int, 2>{}, k + 2);
    advance(std::integral_constant<int, 3>{}, k + 3);
    advance(std::integral_constant<int, 4>{}, k + 4);
    advance(std::integral_constant<int, 5>{}, k + 5);
  }
}

// p.bgr != 0: interleaved 3-channel source (rows hold whole 12-byte groups of 4 pixels: pitch >= 3 * round_up(W, 4))
hipError_t launch_front_o(const FrontParams &p, hipStream_t s)
{
  if (p.chunk_rows < 1 || (unsigned long long)p.H * p.in_pitch >= (1ull << 32)) return hipErrorInvalidValue;
  if (p.prov_out && (unsigned long long)p.H * p.prov_pitch >= (1ull << 32)) return hipErrorInvalidValue;  // (32-bit row offsets into the provisional map)
  if (p.in_pitch < (size_t)(p.bgr ? 3 : 1) * (((size_t)p.W + 3) / 4 * 4)) return hipErrorInvalidValue;
  const dim3 grid((p.total_items + 3) / 4), block(256);
  auto go = [&](auto l2, auto nc) {
    constexpr bool L2 = decltype(l2)::value;
    constexpr int NC = decltype(nc)::value;
    if (p.frame_thr) hipLaunchKernelGGL((k_front_o<L2, NC, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((k_front_o<L2, NC, false>), grid, block, 0, s, p);
  };
  using std::integral_constant;
  if (p.bgr) {
    if (p.l2gradient) go(integral_constant<bool, true>{}, integral_constant<int, 3>{});
    else go(integral_constant<bool, false>{}, integral_constant<int, 3>{});
  } else {
    if (p.l2gradient) go(integral_constant<bool, true>{}, integral_constant<int, 1>{});
    else go(integral_constant<bool, false>{}, integral_constant<int, 1>{});
  }
  return hipGetLastError();
}

// =================================================================================================
// k_copy_rows: pitched device-to-device copy of n frames of `rows` rows of `row_bytes` bytes -- how caller buffers that the
// kernels cannot use in place (pointer / pitch / frame stride not a multiple of 4, rows that do not hold whole pixel
// groups) reach the context's internal pitched buffers and back.  16 bytes per lane, any alignment on either side (the
// hardware takes unaligned global dwordx4 accesses); the row-by-row DMA of hipMemcpy2DAsync moved 512 frames of
// 1918 x 1079 in 1.5 - 2.5 ms each way.
// =================================================================================================
typedef u32 u32x4_any __attribute__((ext_vector_type(4), aligned(1)));
__global__ __launch_bounds__(256) void k_copy_rows(uint8_t *dst, size_t dpitch, size_t dfs, const uint8_t *src, size_t spitch, size_t sfs, unsigned row_bytes, int rows)
{
  const unsigned x = (blockIdx.x * 256u + threadIdx.x) * 16u;
  const int row = blockIdx.y, f = blockIdx.z;
  if (x >= row_bytes || row >= rows) return;
  const uint8_t *q = src + (size_t)f * sfs + (size_t)row * spitch + x;
  uint8_t *d = dst + (size_t)f * dfs + (size_t)row * dpitch + x;
  if (x + 16u <= row_bytes) *reinterpret_cast<u32x4_any *>(d) = *reinterpret_cast<const u32x4_any *>(q);
  else
    for (unsigned k = 0; x + k < row_bytes; ++k) d[k] = q[k];
}

hipError_t launch_copy_rows(void *dst, size_t dpitch, size_t dfs, const void *src, size_t spitch, size_t sfs, size_t row_bytes, int rows, int n, hipStream_t s)
{
  if (row_bytes == 0 || rows <= 0 || n <= 0) return hipSuccess;
  if (row_bytes > 0x7FFFFFFFull || rows > 65535 || n > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((row_bytes + 4095) / 4096), (unsigned)rows, (unsigned)n), block(256);
  hipLaunchKernelGGL(k_copy_rows, grid, block, 0, s, (uint8_t *)dst, dpitch, dfs, (const uint8_t *)src, spitch, sfs, (unsigned)row_bytes, rows);
  return hipGetLastError();
}

// =================================================================================================
// Plain per-stage kernels: the MONO..THRESH taps of CannyEdge::run(finalStage) (cannyEdgeH.cu:58-117).
// One thread per pixel, literal arithmetic; not the fast path.
// =================================================================================================
#define PIX_PROLOG                                              \
  const int col = blockIdx.x * blockDim.x + threadIdx.x;        \
  const int row = blockIdx.y * blockDim.y + threadIdx.y;        \
  const int f = blockIdx.z;                                     \
  if (col >= W || row >= H) return;

__global__ void k_gray(const uint8_t *bgr, size_t bpitch, size_t bfs, uint8_t *mono, size_t mpitch, size_t mfs, int W, int H)
{
  PIX_PROLOG
  const uint8_t *q = bgr + f * bfs + row * bpitch + 3 * col;
  const int v = (q[0] * 7 + q[1] * 38 + q[2] * 19) >> 6;  // cannyEdgeD.cu:17-19,67
  mono[f * mfs + row * mpitch + col] = (uint8_t)min(255, v);
}

__global__ void k_gauss(const uint8_t *mono, size_t mpitch, size_t mfs, uint8_t *blur, size_t bpitch, size_t bfs, int W, int H)
{
  PIX_PROLOG
  blur[f * bfs + row * bpitch + col] = (uint8_t)gauss_chain_px(mono + f * mfs, mpitch, W, H, row, col);
}

__global__ void k_sobel(const uint8_t *blur, size_t bpitch, size_t bfs, int16_t *sx, int16_t *sy, size_t sp, size_t sfs, int W, int H)
{
  PIX_PROLOG
  const uint8_t *b = blur + f * bfs;
  auto at = [&](int r, int c) -> int { return (r >= 0 && r < H && c >= 0 && c < W) ? b[(size_t)r * bpitch + c] : 0; };
  const int x = -at(row - 1, col - 1) + at(row - 1, col + 1) - 2 * at(row, col - 1) + 2 * at(row, col + 1) - at(row + 1, col - 1) + at(row + 1, col + 1);
  const int y = (at(row - 1, col - 1) + 2 * at(row - 1, col) + at(row - 1, col + 1)) - (at(row + 1, col - 1) + 2 * at(row + 1, col) + at(row + 1, col + 1));
  sx[f * sfs + row * sp + col] = (int16_t)x;
  sy[f * sfs + row * sp + col] = (int16_t)y;
}

static __device__ __forceinline__ u32 isqrt_u32(u32 x)
{
  u32 r = (u32)__builtin_sqrtf((float)x);
  while ((u64)r * r > x) --r;
  while ((u64)(r + 1) * (r + 1) <= x) ++r;
  return r;
}

__global__ void k_graddisp(const int16_t *sx, const int16_t *sy, size_t sp, size_t sfs, uint8_t *out, size_t op, size_t ofs, int W, int H)
{
  PIX_PROLOG
  const int x = sx[f * sfs + row * sp + col], y = sy[f * sfs + row * sp + col];
  // float2uchar(min(|grad|,255)) with grad = 4*sqrtf((x/8)^2+(y/8)^2): trunc(grad) = isqrt((x^2+y^2)>>2)
  const u32 g = isqrt_u32((u32)(x * x + y * y) >> 2);
  out[f * ofs + row * op + col] = (uint8_t)min(g, 255u);
}

__global__ void k_nms_tap(const int16_t *sx, const int16_t *sy, size_t sp, size_t sfs, uint8_t *out, size_t op, size_t ofs, int W, int H, int saturate)
{
  PIX_PROLOG
  const int16_t *X = sx + f * sfs, *Y = sy + f * sfs;
  auto S = [&](int r, int c) -> int {
    if (r < 0 || r >= H || c < 0 || c >= W) return 0;
    const int x = X[(size_t)r * sp + c], y = Y[(size_t)r * sp + c];
    return x * x + y * y;
  };
  const int x = X[(size_t)row * sp + col], y = Y[(size_t)row * sp + col];
  const int g = x * x + y * y;
  const int a = abs(x), b = abs(y);
  const int P = 2 * a * b, D = a * a - b * b;
  int bin;
  if (P < abs(D)) bin = D > 0 ? 2 : 0;
  else bin = ((x ^ y) < 0) ? 3 : 1;
  int q, r;
  if (bin == 0) { q = S(row + 1, col); r = S(row - 1, col); }
  else if (bin == 1) { q = S(row + 1, col - 1); r = S(row - 1, col + 1); }
  else if (bin == 2) { q = S(row, col + 1); r = S(row, col - 1); }
  else { q = S(row - 1, col - 1); r = S(row + 1, col + 1); }
  const bool keep = q <= g && r <= g;
  const u32 gt = isqrt_u32((u32)g >> 2);
  out[f * ofs + row * op + col] = keep ? (uint8_t)(saturate ? min(gt, 255u) : (gt & 0xFFu)) : 0;
}

__global__ void k_thresh(const uint8_t *nms, size_t np, size_t nfs, uint8_t *out, size_t op, size_t ofs, int W, int H, int low, int high)
{
  PIX_PROLOG
  const int v = nms[f * nfs + row * np + col];
  out[f * ofs + row * op + col] = v > high ? 255 : v > low ? 128 : 0;
}

#define PIX_GRID dim3 blk(64, 4, 1), grd((W + 63) / 64, (H + 3) / 4, n)
hipError_t launch_gray(const uint8_t *bgr, size_t bpitch, size_t bfs, uint8_t *mono, size_t mpitch, size_t mfs, int W, int H, int n, hipStream_t s)
{ PIX_GRID; hipLaunchKernelGGL(k_gray, grd, blk, 0, s, bgr, bpitch, bfs, mono, mpitch, mfs, W, H); return hipGetLastError(); }
hipError_t launch_gauss(const uint8_t *mono, size_t mpitch, size_t mfs, uint8_t *blur, size_t bpitch, size_t bfs, int W, int H, int n, hipStream_t s)
{ PIX_GRID; hipLaunchKernelGGL(k_gauss, grd, blk, 0, s, mono, mpitch, mfs, blur, bpitch, bfs, W, H); return hipGetLastError(); }
hipError_t launch_sobel(const uint8_t *blur, size_t bpitch, size_t bfs, int16_t *sx, int16_t *sy, size_t sp, size_t sfs, int W, int H, int n, hipStream_t s)
{ PIX_GRID; hipLaunchKernelGGL(k_sobel, grd, blk, 0, s, blur, bpitch, bfs, sx, sy, sp, sfs, W, H); return hipGetLastError(); }
hipError_t launch_graddisp(const int16_t *sx, const int16_t *sy, size_t sp, size_t sfs, uint8_t *out, size_t op, size_t ofs, int W, int H, int n, hipStream_t s)
{ PIX_GRID; hipLaunchKernelGGL(k_graddisp, grd, blk, 0, s, sx, sy, sp, sfs, out, op, ofs, W, H); return hipGetLastError(); }
hipError_t launch_nms(const int16_t *sx, const int16_t *sy, size_t sp, size_t sfs, uint8_t *out, size_t op, size_t ofs, int W, int H, int n, int saturate, hipStream_t s)
{ PIX_GRID; hipLaunchKernelGGL(k_nms_tap, grd, blk, 0, s, sx, sy, sp, sfs, out, op, ofs, W, H, saturate); return hipGetLastError(); }
hipError_t launch_thresh(const uint8_t *nms, size_t np, size_t nfs, uint8_t *out, size_t op, size_t ofs, int W, int H, int n, int low, int high, hipStream_t s)
{ PIX_GRID; hipLaunchKernelGGL(k_thresh, grd, blk, 0, s, nms, np, nfs, out, op, ofs, W, H, low, high); return hipGetLastError(); }

}  // namespace hc
