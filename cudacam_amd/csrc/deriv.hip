// deriv.hip -- k_deriv16: the derivatives cv::Canny computes before its NMS, on their own.
//
//   u8 frames (1 or 3 interleaved channels) -> int16 dx / dy planes with the same interleave (CV_16SC1 / CV_16SC3), the
//   layout hc_run_gradients_device reads.  Sobel(src, CV_16S, 1, 0 / 0, 1, ksize, scale, 0, BORDER_REPLICATE) restated:
//     ksize  3   smoothing [1 2 1]               derivative [-1 0 1]              scale 1
//     ksize  5             [1 4 6 4 1]                      [-1 -2 0 2 1]         scale 1
//     ksize  7             [1 6 15 20 15 6 1]               [-1 -4 -5 0 5 4 1]    scale 1/16, rounded half to even
//     ksize -1 (Scharr)    [3 10 3]                         [-1 0 1]              scale 1
//   a correlation, dx = derivative taps along x and smoothing taps along y, dy the other way round.
// Layout as k_front_o_ext's Source A: a wave owns a 248-column strip, lane l the 4 pixels at strip * 248 - 4 + 4 l, lanes 0
// and 63 are halo; columns replicate through a per-lane byte selector, rows by clamping the row index.  The horizontal
// passes run in packed int16 pairs (every horizontal partial fits int16 for all four kinds) and stay in a register ring of
// ksize rows; the vertical pass is packed too, except at ksize 7, whose sums (|S| <= 163200) need 32 bits before the
// division.  A work item is (frame, strip, DERIV_CHUNK_ROWS rows) with a warm-up of ksize - 1 rows.  Registers only.
// Memory: no byte outside [row, row + C W) of an input row is read, none outside [row, row + 2 C W) of an output row is
// written, at any alignment: dword loads only for whole 4-pixel groups of 4-aligned rows (byte loads otherwise), 8- or
// 4-byte stores only for whole groups of rows aligned that far (int16 stores otherwise).
#include "canny_device.h"

namespace hc {

namespace {

typedef short i16x2v __attribute__((ext_vector_type(2)));
typedef u32 u32x2v __attribute__((ext_vector_type(2)));
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

template <int KIND, int NC>
__global__ __launch_bounds__(256) void k_deriv16(const DerivParams p)
{
  constexpr int K = deriv_taps(KIND), R = K / 2;
  constexpr bool WIDE = KIND == 7;  // 32-bit vertical sums, then / 16 half to even
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const int item = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + wib);
  if (item >= p.total_items) return;
  const int chunk = item % p.nchunks;
  const int strip = (item / p.nchunks) % p.nstrips;
  const int frame = item / (p.nchunks * p.nstrips);
  const int W = p.W, H = p.H;
  const int r0 = chunk * DERIV_CHUNK_ROWS, rend = min(r0 + DERIV_CHUNK_ROWS, H);
  const int c0 = strip * DERIV_STRIP_W - STRIP_HALO + lane * PX_PER_LANE;
  const int rlast = min(H - 1, rend - 1 + R);  // last source row this item needs

  // BORDER_REPLICATE: rows by clamping, columns by a per-lane byte selector over the 4-pixel group that holds the lane's
  // first (clamped) column
  const int cl0 = min(max(c0, 0), W - 1);
  const int ld_col = cl0 & ~3;
  u32 rsel = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) rsel |= (u32)(min(max(c0 + k, 0), W - 1) - ld_col) << (8 * k);
  const bool fast_ld = p.in_aligned && ld_col + 4 <= W;  // the whole group lies inside the row, the row is 4-aligned
  const int last_byte = NC * W - 1;
  const uint8_t *fbase = p.in + (size_t)frame * p.in_frame_stride;
  struct Raw { u32 d[NC]; };
  auto load_row = [&](int row) -> Raw {
    const int rr = min(max(row, 0), rlast);
    const uint8_t *rp = fbase + (size_t)rr * p.in_pitch;
    Raw r;
    if (fast_ld) {
      const u32 *q = reinterpret_cast<const u32 *>(rp + NC * ld_col);
#pragma unroll
      for (int i = 0; i < NC; ++i) r.d[i] = q[i];
    } else {  // bytes past the row's end are never selected (rsel): they read as the row's last byte
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        u32 v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) v |= (u32)rp[min(NC * ld_col + 4 * i + b, last_byte)] << (8 * b);
        r.d[i] = v;
      }
    }
    return r;
  };
  // channel ch of the lane's 4 pixels as one dword, replicated at the borders
  auto use_row = [&](const Raw &raw, int ch) -> u32 {
    u32 v = raw.d[0];
    if constexpr (NC == 3) {
      const u32 selA = ch == 0 ? 0x0c060300u : ch == 1 ? 0x0c070401u : 0x0c0c0502u;
      const u32 selB = ch == 0 ? 0x05020100u : ch == 1 ? 0x06020100u : 0x07040100u;
      v = __builtin_amdgcn_perm(raw.d[NC > 2 ? 2 : 0], __builtin_amdgcn_perm(raw.d[NC > 1 ? 1 : 0], raw.d[0], selA), selB);
    }
    return __builtin_amdgcn_perm(0u, v, rsel);
  };

  // per channel: horizontal derivative / smoothing rows of the last K source rows, packed pairs [ring][pair]
  u32 HD[NC][K][2], HS[NC][K][2];
#pragma unroll
  for (int ch = 0; ch < NC; ++ch)
#pragma unroll
    for (int a = 0; a < K; ++a) HD[ch][a][0] = HD[ch][a][1] = HS[ch][a][0] = HS[ch][a][1] = 0;

  const bool st_lane = lane >= 1 && lane <= 62 && c0 < W;
  const bool st_full = c0 + 3 < W;
  const size_t out_off = (size_t)frame * p.frame_stride + (size_t)(2 * NC) * (size_t)max(c0, 0);
  uint8_t *const xbase = p.dx + out_off, *const ybase = p.dy + out_off;
  const int out_align = p.out_align;
  const int n_el = NC * min(4, W - c0);  // int16 elements of the lane that lie inside the row (partial groups)
  auto store_row = [&](uint8_t *q, const u32 (&w)[2 * NC]) {
    if (st_full && out_align >= 8) {
#pragma unroll
      for (int j = 0; j < NC; ++j) reinterpret_cast<u32x2v *>(q)[j] = u32x2v{ w[2 * j], w[2 * j + 1] };
    } else if (st_full && out_align >= 4) {
#pragma unroll
      for (int j = 0; j < 2 * NC; ++j) reinterpret_cast<u32 *>(q)[j] = w[j];
    } else {
      unsigned short *h = reinterpret_cast<unsigned short *>(q);
#pragma unroll
      for (int e = 0; e < 4 * NC; ++e)
        if (e < n_el) h[e] = (unsigned short)(w[e >> 1] >> (16 * (e & 1)));
    }
  };

  // one step: source row k arrives -> output row g = k - R
  auto step = [&](auto uc, int k, const Raw &raw) {
    constexpr int u = decltype(uc)::value;
    const int g = k - R;
    const bool emit = g >= r0 && g < rend;  // wave-uniform
    u32 X[NC][2], Y[NC][2];                 // per channel: (px 0, px 1), (px 2, px 3)
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
      // horizontal pass on the new row.  P[t + 4] = the pixel pair that starts t columns from the lane's first
      const u32 b = use_row(raw, ch);
      u32 P[11];
      P[4] = unpack_lo(b); P[6] = unpack_hi(b);
      P[2] = from_lane_below(P[6]); P[8] = from_lane_above(P[4]);
      P[0] = from_lane_below(P[4]); P[10] = from_lane_above(P[6]);
      P[1] = pair_shift(P[2], P[0]); P[3] = pair_shift(P[4], P[2]); P[5] = pair_shift(P[6], P[4]);
      P[7] = pair_shift(P[8], P[6]); P[9] = pair_shift(P[10], P[8]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = 4 + 2 * h;
        i16x2v hs = V(P[c]) * splat(smooth_tap(KIND, R)), hd = splat(0);
#pragma unroll
        for (int t = 0; t < R; ++t) {
          hs += (V(P[c - R + t]) + V(P[c + R - t])) * splat(smooth_tap(KIND, t));
          hd += (V(P[c + R - t]) - V(P[c - R + t])) * splat(deriv_tap(KIND, K - 1 - t));
        }
        HS[ch][u][h] = W32(hs);
        HD[ch][u][h] = W32(hd);
      }
      if (emit) {
        // vertical pass over source rows k - K + 1 .. k: ring slot of tap t (t = 0: the oldest row) is (u + 1 + t) % K
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if constexpr (!WIDE) {
            i16x2v vx = V(HD[ch][(u + 1 + R) % K][h]) * splat(smooth_tap(KIND, R)), vy = splat(0);
#pragma unroll
            for (int t = 0; t < R; ++t) {
              const int so = (u + 1 + t) % K, sn = (u + K - t) % K;  // rows g - R + t and g + R - t
              vx += (V(HD[ch][so][h]) + V(HD[ch][sn][h])) * splat(smooth_tap(KIND, t));
              vy += (V(HS[ch][sn][h]) - V(HS[ch][so][h])) * splat(deriv_tap(KIND, K - 1 - t));
            }
            X[ch][h] = W32(vx);
            Y[ch][h] = W32(vy);
          } else {
            // symmetric rows first, still packed (|hd| <= 2550, hs <= 16320: sums and differences fit int16), then 32 bits
            const u32 mid = HD[ch][(u + 1 + R) % K][h];
            int sx0 = lo16(mid) * smooth_tap(KIND, R), sx1 = hi16(mid) * smooth_tap(KIND, R), sy0 = 0, sy1 = 0;
#pragma unroll
            for (int t = 0; t < R; ++t) {
              const int so = (u + 1 + t) % K, sn = (u + K - t) % K;
              const u32 a = W32(V(HD[ch][so][h]) + V(HD[ch][sn][h]));
              const u32 d = W32(V(HS[ch][sn][h]) - V(HS[ch][so][h]));
              sx0 += lo16(a) * smooth_tap(KIND, t); sx1 += hi16(a) * smooth_tap(KIND, t);
              sy0 += lo16(d) * deriv_tap(KIND, K - 1 - t); sy1 += hi16(d) * deriv_tap(KIND, K - 1 - t);
            }
            // S / 16 rounded half to even (what cvRound gives for the exact float S / 16)
            auto rnd = [](int s) -> u32 { return (u32)((s + 7 + ((s >> 4) & 1)) >> 4); };
            X[ch][h] = (rnd(sx0) & 0xFFFFu) | (rnd(sx1) << 16);
            Y[ch][h] = (rnd(sy0) & 0xFFFFu) | (rnd(sy1) << 16);
          }
        }
      }
    }
    if (emit && st_lane) {
      u32 wx[2 * NC], wy[2 * NC];
      if constexpr (NC == 1) {
        wx[0] = X[0][0]; wx[1] = X[0][1];
        wy[0] = Y[0][0]; wy[1] = Y[0][1];
      } else {
        // interleave: element 3 q + ch
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          wx[3 * h + 0] = pick2<0, 0>(X[0][h], X[1][h]); wx[3 * h + 1] = pick2<0, 1>(X[2][h], X[0][h]); wx[3 * h + 2] = pick2<1, 1>(X[1][h], X[2][h]);
          wy[3 * h + 0] = pick2<0, 0>(Y[0][h], Y[1][h]); wy[3 * h + 1] = pick2<0, 1>(Y[2][h], Y[0][h]); wy[3 * h + 2] = pick2<1, 1>(Y[1][h], Y[2][h]);
        }
      }
      const size_t roff = (size_t)g * p.pitch;
      store_row(xbase + roff, wx);
      store_row(ybase + roff, wy);
    }
  };

  // source rows r0 - R .. rend - 1 + R, K steps per loop trip (the ring period); a row is requested K steps before it is used
  const int k0 = r0 - R, kend = rend + R;
  Raw bn[K];
#pragma unroll
  for (int j = 0; j < K; ++j) bn[j] = load_row(k0 + j);
  auto advance = [&](auto uc, int k) {
    constexpr int j = decltype(uc)::value;
    const Raw b = bn[j];
    bn[j] = load_row(k + K);
    step(uc, k, b);
  };
#pragma nounroll
  for (int k = k0; k < kend; k += K) {
    advance(std::integral_constant<int, 0>{}, k + 0);
    advance(std::integral_constant<int, 1>{}, k + 1);
    advance(std::integral_constant<int, 2>{}, k + 2);
    if constexpr (K > 3) {
      advance(std::integral_constant<int, 3>{}, k + 3);
      advance(std::integral_constant<int, 4>{}, k + 4);
    }
    if constexpr (K > 5) {
      advance(std::integral_constant<int, 5>{}, k + 5);
      advance(std::integral_constant<int, 6>{}, k + 6);
    }
  }
}

template <int KIND>
void launch_kind(const DerivParams &p, const dim3 grid, const dim3 block, hipStream_t s)
{
  if (p.channels == 3) hipLaunchKernelGGL((k_deriv16<KIND, 3>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((k_deriv16<KIND, 1>), grid, block, 0, s, p);
}

}  // namespace

hipError_t launch_deriv16(const DerivParams &p, hipStream_t s)
{
  if (p.W < 1 || p.H < 1 || p.nframes < 1 || (p.channels != 1 && p.channels != 3) || !deriv_ksize_ok(p.ksize) || !p.in || !p.dx || !p.dy
      || (((uintptr_t)p.dx | (uintptr_t)p.dy | p.pitch | p.frame_stride) & 1u) || p.in_pitch < (size_t)p.channels * p.W
      || p.pitch < (size_t)2 * p.channels * p.W || p.nstrips != deriv_strips(p.W) || p.nchunks != deriv_chunks(p.H)
      || (long long)p.total_items != (long long)p.nframes * p.nstrips * p.nchunks)
    return hipErrorInvalidValue;
  const dim3 grid((p.total_items + 3) / 4), block(256);
  switch (p.ksize) {
  case 3: launch_kind<3>(p, grid, block, s); break;
  case 5: launch_kind<5>(p, grid, block, s); break;
  case 7: launch_kind<7>(p, grid, block, s); break;
  default: launch_kind<-1>(p, grid, block, s); break;
  }
  return hipGetLastError();
}

}  // namespace hc
