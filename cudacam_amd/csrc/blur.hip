// blur.hip -- k_gauss8: cv::GaussianBlur's fixed-point path for CV_8U as hc_gaussian_blur_device states it.
//
//   u8 frames (1 or 3 interleaved channels) -> u8 frames with the same interleave: a separable K x K correlation, K = 3, 5
//   or 7, the same K Q8 taps t (each <= 256, sum 256; wave-uniform, by value in the parameter block) along x and y:
//   h = sum t[i] src (exact in u16: <= 255 * 256), v = sum t[j] h (exact in u32: < 2^24), out = (v + 32768) >> 16.
// Layout as k_deriv16: a wave owns a 248-column strip, lane l the 4 pixels at strip * 248 - 4 + 4 l, lanes 0 and 63 are
// halo (the 7-tap filter needs 3 of their 4 columns).  The horizontal sums of the last K rows stay in a register ring per
// channel, as packed u16 pairs; rows are requested K steps ahead.  A work item is (frame, strip, BLUR_CHUNK_ROWS rows) with a
// warm-up of K - 1 rows.  No LDS, no atomics, registers only; every ring slot is a compile-time index.
// Borders (border_index, canny_params.h: reflect-101 or replicate, also for axes shorter than the radius): rows by mapping
// the row index before the load, warm-up rows included.  Columns: a lane holds the pixels of its 4 columns AS MAPPED, so its
// neighbours' windows need no further care -- the lanes whose 4 columns all lie inside the row load them as a group, the few
// per strip with a column outside it (and within the radius of it) gather their 4 columns bytewise by mapped index, under
// either border; lanes further out load nothing.
// Memory: no byte outside [row, row + C W) of an input or output row is read or written, at any alignment: dword loads and
// stores only for whole 4-pixel groups of 4-aligned rows (in_aligned / out_aligned), bytes otherwise.  Rows are addressed
// with 32-bit offsets (H * pitch < 2^32 on both sides: plan_gaussian_blur).
#include "sep_deriv.h"

namespace hc {

namespace {

using namespace sep;

// acc + (half HA of the packed u16 pair a) * (low half of t), in 32 bits
template <int HA>
static __device__ __forceinline__ u32 mad_u16(u32 a, u32 t, u32 acc)
{
  u32 d;
  if (HA == 0) asm("v_mad_u32_u16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(t), "v"(acc));
  else asm("v_mad_u32_u16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(d) : "v"(a), "s"(t), "v"(acc));
  return d;
}

template <int K, int NC>
__global__ __launch_bounds__(256) void k_gauss8(const BlurParams p)
{
  constexpr int RAD = K / 2;
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const int item = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + wib);
  if (item >= p.total_items) return;
  const int chunk = item % p.nchunks;
  const int strip = (item / p.nchunks) % p.nstrips;
  const int frame = item / (p.nchunks * p.nstrips);
  const int W = p.W, H = p.H, border = p.border;
  const int r0 = chunk * BLUR_CHUNK_ROWS, rend = min(r0 + BLUR_CHUNK_ROWS, H);
  const int c0 = strip * BLUR_STRIP_W - STRIP_HALO + lane * PX_PER_LANE;
  const int vlast = rend - 1 + RAD;  // last (unmapped) source row this item needs

  // the taps, wave-uniform: as they are for the 32-bit vertical pass, both halves for the packed horizontal one
  u32 t1[K], t2[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    t1[i] = (u32)__builtin_amdgcn_readfirstlane((int)p.taps[i]);
    t2[i] = t1[i] * 0x10001u;
  }

  // columns: `inside` lanes own 4 columns of the row; `edge` lanes have one outside it that a window may reach
  const bool inside = c0 >= 0 && c0 + 3 < W;
  const bool edge = !inside && c0 + 3 >= -RAD && c0 <= W - 1 + RAD;
  const bool fast_ld = inside && p.in_aligned;
  const bool byte_ld = (inside || edge) && !fast_ld;
  u32 boff[4] = { 0, 0, 0, 0 };  // byte offset in the row of channel 0 of the lane's 4 (mapped) columns
  if (byte_ld) {
#pragma unroll
    for (int k = 0; k < 4; ++k) boff[k] = (u32)(NC * border_index(c0 + k, W, border));
  }
  const uint8_t *fbase = p.in + (size_t)frame * p.in_frame_stride;
  const u32 in_pitch = (u32)p.in_pitch;
  struct Raw { u32 d[NC]; };  // the lane's 4 pixels as they lie in memory: 4 NC interleaved bytes
  auto load_row = [&](int vrow) -> Raw {
    const int rr = border_index(min(vrow, vlast), H, border);  // wave-uniform
    const uint8_t *rp = fbase + (u32)rr * in_pitch;
    Raw r;
#pragma unroll
    for (int i = 0; i < NC; ++i) r.d[i] = 0;
    if (fast_ld) {
      const u32 *q = reinterpret_cast<const u32 *>(rp + NC * c0);
#pragma unroll
      for (int i = 0; i < NC; ++i) r.d[i] = q[i];
    } else if (byte_ld) {
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        u32 v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) v |= (u32)rp[boff[(4 * i + b) / NC] + (u32)((4 * i + b) % NC)] << (8 * b);
        r.d[i] = v;
      }
    }
    return r;
  };
  // channel ch of the 4 pixels as one dword: of 12 interleaved bytes the channel's (ch, ch + 3, ch + 6, ch + 9)
  auto channel_of = [](const u32 (&d)[NC], int ch) -> u32 {
    if constexpr (NC == 1) return d[0];
    else {
      const u32 selA = ch == 0 ? 0x0c060300u : ch == 1 ? 0x0c070401u : 0x0c0c0502u;
      const u32 selB = ch == 0 ? 0x05020100u : ch == 1 ? 0x06020100u : 0x07040100u;
      return __builtin_amdgcn_perm(d[2], __builtin_amdgcn_perm(d[1], d[0], selA), selB);
    }
  };

  // per channel: the horizontal sums of the last K source rows, packed u16 pairs [ring][pair]
  u32 HR[NC][K][2];
#pragma unroll
  for (int ch = 0; ch < NC; ++ch)
#pragma unroll
    for (int a = 0; a < K; ++a) HR[ch][a][0] = HR[ch][a][1] = 0;

  const bool st_lane = lane >= 1 && lane <= 62 && c0 < W;
  const bool st_fast = c0 + 3 < W && p.out_aligned;
  uint8_t *const obase = p.out + (size_t)frame * p.out_frame_stride + (size_t)NC * (size_t)max(c0, 0);
  const u32 out_pitch = (u32)p.out_pitch;
  const int n_el = NC * min(4, W - c0);  // bytes of the lane that lie inside the row (partial groups)
  const u32 half = 32768u;

  // one step: source row k arrives -> output row g = k - RAD
  auto step = [&](auto uc, int k, const Raw &raw) {
    constexpr int u = decltype(uc)::value;
    const int g = k - RAD;
    const bool emit = g >= r0 && g < rend;  // wave-uniform
    u32 B[NC];                              // per channel: the 4 output pixels
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
      const PairWindow P = sep_window(channel_of(raw.d, ch));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = 4 + 2 * h;
        u16x2 s = U(P.p[c - RAD]) * U(t2[0]);
#pragma unroll
        for (int i = 1; i < K; ++i) s += U(P.p[c - RAD + i]) * U(t2[i]);
        HR[ch][u][h] = R(s);
      }
      if (emit) {  // vertical pass over source rows k - K + 1 .. k: tap j takes ring slot (u + 1 + j) % K
        u32 a[4] = { half, half, half, half };
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const int slot = (u + 1 + j) % K;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            a[2 * h] = mad_u16<0>(HR[ch][slot][h], t1[j], a[2 * h]);
            a[2 * h + 1] = mad_u16<1>(HR[ch][slot][h], t1[j], a[2 * h + 1]);
          }
        }
        // (v + 32768) >> 16 is byte 2 of each sum (below 2^24)
        const u32 lo = __builtin_amdgcn_perm(a[1], a[0], 0x0c0c0602u), hi = __builtin_amdgcn_perm(a[3], a[2], 0x06020c0cu);
        B[ch] = lo | hi;
      }
    }
    if (emit && st_lane) {
      u32 w[NC];
      if constexpr (NC == 1) w[0] = B[0];
      else {  // interleave: byte 3 q + ch
        w[0] = __builtin_amdgcn_perm(B[2], __builtin_amdgcn_perm(B[1], B[0], 0x010c0400u), 0x03040100u);
        w[1] = __builtin_amdgcn_perm(B[2], __builtin_amdgcn_perm(B[1], B[0], 0x06020c05u), 0x03020500u);
        w[2] = __builtin_amdgcn_perm(B[2], __builtin_amdgcn_perm(B[1], B[0], 0x0c07030cu), 0x07020106u);
      }
      uint8_t *q = obase + (u32)g * out_pitch;
      if (st_fast) {
#pragma unroll
        for (int j = 0; j < NC; ++j) reinterpret_cast<u32 *>(q)[j] = w[j];
      } else {
#pragma unroll
        for (int e = 0; e < 4 * NC; ++e)
          if (e < n_el) q[e] = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
      }
    }
  };

  // source rows r0 - RAD .. rend - 1 + RAD, K steps per loop trip (the ring period); a row is requested K steps before it is used
  const int k0 = r0 - RAD, kend = rend + RAD;
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

template <int K>
void launch_k(const BlurParams &p, const dim3 grid, const dim3 block, hipStream_t s)
{
  if (p.channels == 3) hipLaunchKernelGGL((k_gauss8<K, 3>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((k_gauss8<K, 1>), grid, block, 0, s, p);
}

}  // namespace

hipError_t launch_gauss8(const BlurParams &p, hipStream_t s)
{
  unsigned sum = 0;
  for (int i = 0; i < BLUR_MAX_TAPS; ++i) sum += p.taps[i] <= 256 && (i < p.ksize || !p.taps[i]) ? p.taps[i] : 1000u;
  if (p.W < 1 || p.H < 1 || p.nframes < 1 || (p.channels != 1 && p.channels != 3) || !blur_ksize_ok(p.ksize) || sum != 256 || !p.in || !p.out
      || (p.border != BLUR_REFLECT_101 && p.border != BLUR_REPLICATE) || p.in_pitch < (size_t)p.channels * p.W || p.out_pitch < (size_t)p.channels * p.W
      || p.in_pitch > 0xFFFFFFFFull / (size_t)p.H || p.out_pitch > 0xFFFFFFFFull / (size_t)p.H || p.nstrips != blur_strips(p.W) || p.nchunks != blur_chunks(p.H)
      || (long long)p.total_items != (long long)p.nframes * p.nstrips * p.nchunks)
    return hipErrorInvalidValue;
  const dim3 grid((p.total_items + 3) / 4), block(256);
  switch (p.ksize) {
  case 3: launch_k<3>(p, grid, block, s); break;
  case 5: launch_k<5>(p, grid, block, s); break;
  default: launch_k<7>(p, grid, block, s); break;
  }
  return hipGetLastError();
}

}  // namespace hc
