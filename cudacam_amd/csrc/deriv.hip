// deriv.hip -- k_deriv16: the derivatives cv::Canny computes before its NMS, on their own.
//
//   u8 frames (1 or 3 interleaved channels) -> int16 dx / dy planes with the same interleave (CV_16SC1 / CV_16SC3), the
//   layout hc_run_gradients_device reads: cv::Sobel at ksize 3, 5, 7 or -1 (Scharr), the taps and both passes of sep_deriv.h.
// Layout as k_front_o_ext's u8 sources: a wave owns a 248-column strip, lane l the 4 pixels at strip * 248 - 4 + 4 l, lanes 0
// and 63 are halo; columns replicate through a per-lane byte selector, rows by clamping the row index.  The horizontal
// passes stay in a register ring of ksize rows.  A work item is (frame, strip, DERIV_CHUNK_ROWS rows) with a warm-up of
// ksize - 1 rows.  Registers only.
// Memory: no byte outside [row, row + C W) of an input row is read, none outside [row, row + 2 C W) of an output row is
// written, at any alignment: dword loads only for whole 4-pixel groups of 4-aligned rows (byte loads otherwise), 8- or
// 4-byte stores only for whole groups of rows aligned that far (int16 stores otherwise).
#include "sep_deriv.h"

namespace hc {

namespace {

using namespace sep;

typedef u32 u32x2v __attribute__((ext_vector_type(2)));

template <int KIND, int NC>
__global__ __launch_bounds__(256) void k_deriv16(const DerivParams p)
{
  constexpr int K = deriv_taps(KIND), R = K / 2;
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
      const PairWindow P = sep_window(pick_channel(raw.d, ch, rsel));
#pragma unroll
      for (int h = 0; h < 2; ++h) sep_hpass<KIND>(P, h, HD[ch][u][h], HS[ch][u][h]);
      if (emit) {  // vertical pass over source rows k - K + 1 .. k
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if constexpr (KIND != 7) sep_vpass_pk<KIND, K, u>(HD[ch], HS[ch], h, X[ch][h], Y[ch][h]);
          else {
            int x0, x1, y0, y1;
            sep_vpass_wide<K, u>(HD[ch], HS[ch], h, x0, x1, y0, y1);
            X[ch][h] = ((u32)x0 & 0xFFFFu) | ((u32)x1 << 16);
            Y[ch][h] = ((u32)y0 & 0xFFFFu) | ((u32)y1 << 16);
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
