// flow.hip -- the kernels of hc_pyr_down_device and hc_lk_flow_device: cv::pyrDown of u8 planes and one pyramid level of
// cv::calcOpticalFlowPyrLK on corner lists (the contract is stated in include/hipcanny.h and restated in tests/flow_ref.py).
//
//   k_pyr_down8     the lane layout of k_gauss8 on the source plane: a wave owns a strip of 248 source columns, lane l the 4 source
//                   pixels at strip * 248 - 4 + 4 l -- the centres of its 2 destination pixels are the first and the third of them
//                   --, lanes 0 and 63 are halo.  Per source row the 5-tap sums at stride 2 of the lane's two destination columns,
//                   one packed u16 pair (<= 16 * 255): the columns left and right of the lane's come from its neighbours by DPP.  The
//                   sums of the five source rows around a destination row stay in registers; two rows arrive per destination row, so
//                   every source row is read once per work item.  The vertical sum + 128 still fits u16 (<= 65408): packed as well.
//                   Borders as k_gauss8: rows by mapping the row index before the load, columns by holding a lane's 4 pixels AS
//                   MAPPED (reflect-101), the few lanes per strip with a column outside the row gathering bytewise.
//   k_lk_flow<NR>   one wave per (frame, point), NR rounds of 64 window pixels: lane l owns the pixels t = l + 64 r, r < NR, at
//                   (t % win, t / win) of the window; those with t >= win^2 are idle.  The template (I, gx, gy as int16) is made once
//                   from a clamped 4 x 4 patch of `prev` per pixel and stays in 2 registers a round; an iteration gathers the 4
//                   neighbours of each pixel in `next` again and nothing else.  Lane sums fit int32 (16 products below 2^25); the wave
//                   sums are int64, by four DPP steps inside the rows of 16 lanes and scalar adds of the four rows, so they arrive in
//                   SGPRs and the 2 x 2 solve is uniform.  No LDS, no atomics, no global scratch.
// Every float step of the contract is one rounded float32 operation (__fmul_rn and its kin; this file is compiled with
// -ffp-contract=off, and says so itself below); the root is __builtin_sqrtf and the divisions are IEEE (see corners.hip).
#include "sep_deriv.h"

#pragma clang fp contract(off)

namespace hc {

namespace {

using namespace sep;

// ---- hc_pyr_down_device ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_pyr_down8(const PyrParams p)
{
  const int lane = threadIdx.x & 63;
  const int item = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (int)(threadIdx.x >> 6));
  if (item >= p.total_items) return;
  const int chunk = item % p.nchunks;
  const int strip = (item / p.nchunks) % p.nstrips;
  const int frame = item / (p.nchunks * p.nstrips);
  const int W = p.W, H = p.H, dW = p.dW;
  const int r0 = chunk * PYR_CHUNK_ROWS, rend = min(r0 + PYR_CHUNK_ROWS, p.dH);  // destination rows
  const int c0 = strip * PYR_STRIP_W - STRIP_HALO + lane * PX_PER_LANE;          // source column
  const int vlast = 2 * (rend - 1) + 2;  // last (unmapped) source row this item needs

  // columns: `inside` lanes own 4 columns of the row; `edge` lanes have one outside it that a window may reach (radius 2)
  const bool inside = c0 >= 0 && c0 + 3 < W;
  const bool edge = !inside && c0 + 3 >= -2 && c0 <= W - 1 + 2;
  const bool fast_ld = inside && p.in_aligned;
  const bool byte_ld = (inside || edge) && !fast_ld;
  u32 boff[4] = { 0, 0, 0, 0 };  // the lane's 4 (mapped) columns
  if (byte_ld) {
#pragma unroll
    for (int k = 0; k < 4; ++k) boff[k] = (u32)border_index(c0 + k, W, BLUR_REFLECT_101);
  }
  const uint8_t *fbase = p.in + (size_t)frame * p.in_frame_stride;
  const u32 in_pitch = (u32)p.in_pitch;
  auto load_row = [&](int vrow) -> u32 {
    const int rr = border_index(min(vrow, vlast), H, BLUR_REFLECT_101);  // wave-uniform
    const uint8_t *rp = fbase + (u32)rr * in_pitch;                      // (H * pitch < 2^32)
    u32 v = 0;
    if (fast_ld) v = *reinterpret_cast<const u32 *>(rp + c0);
    else if (byte_ld) {
#pragma unroll
      for (int b = 0; b < 4; ++b) v |= (u32)rp[boff[b]] << (8 * b);
    }
    return v;
  };
  // the 5-tap sums of the lane's two destination columns: centres at its pixels 0 and 2, as one packed u16 pair
  auto hsum = [&](u32 raw) -> u32 {
    const u32 p0 = unpack_lo(raw), p2 = unpack_hi(raw);                // columns (0, 1), (2, 3)
    const u32 pm = from_lane_below(p2), pp = from_lane_above(p0);      // columns (-2, -1), (4, 5)
    const u16x2 e0 = U(pick2<0, 0>(pm, p0)), e1 = U(pick2<1, 1>(pm, p0)), e2 = U(pick2<0, 0>(p0, p2)), e3 = U(pick2<1, 1>(p0, p2)), e4 = U(pick2<0, 0>(p2, pp));
    const u16x2 four = { 4, 4 }, six = { 6, 6 };
    return R((u16x2)((e0 + e4) + (e1 + e3) * four + e2 * six));
  };

  const bool st_lane = lane >= 1 && lane <= 62 && c0 < W;
  const int d0 = max(c0, 0) >> 1;  // the lane's first destination column
  const bool st_two = d0 + 1 < dW;
  const bool st_fast = st_two && p.out_aligned;
  uint8_t *const obase = p.out + (size_t)frame * p.out_frame_stride + (size_t)d0;
  const u32 out_pitch = (u32)p.out_pitch;

  // the sums of the source rows 2 y - 2, 2 y - 1, 2 y are carried over from the row before; 2 y + 1 and 2 y + 2 arrive
  u32 ha, hb, hc, hd, he;
  hc = hsum(load_row(2 * r0 - 2));
  hd = hsum(load_row(2 * r0 - 1));
  he = hsum(load_row(2 * r0));
  u32 n1 = load_row(2 * r0 + 1), n2 = load_row(2 * r0 + 2);
#pragma nounroll
  for (int y = r0; y < rend; ++y) {
    const u32 raw1 = n1, raw2 = n2;
    n1 = load_row(2 * y + 3);  // requested one destination row ahead
    n2 = load_row(2 * y + 4);
    ha = hc; hb = hd; hc = he;
    hd = hsum(raw1);
    he = hsum(raw2);
    const u16x2 four = { 4, 4 }, six = { 6, 6 }, half = { 128, 128 };
    const u32 v = R((u16x2)((U(ha) + U(he)) + (U(hb) + U(hd)) * four + U(hc) * six + half));  // <= 65408: no carry between the halves
    if (st_lane) {
      uint8_t *q = obase + (u32)y * out_pitch;  // (dH * out_pitch < 2^32)
      const u32 two = __builtin_amdgcn_perm(0u, v, 0x0c0c0301u);  // (v >> 8) of both halves as two bytes
      if (st_fast) *reinterpret_cast<unsigned short *>(q) = (unsigned short)two;
      else {
        q[0] = (uint8_t)two;
        if (st_two) q[1] = (uint8_t)(two >> 8);
      }
    }
  }
}

// ---- hc_lk_flow_device ----------------------------------------------------------------------------

template <int CTRL>
static __device__ __forceinline__ long long i64_dpp(long long v)
{
  const u32 lo = (u32)__builtin_amdgcn_update_dpp(0, (int)(u32)v, CTRL, 0xF, 0xF, true);
  const u32 hi = (u32)__builtin_amdgcn_update_dpp(0, (int)(u32)((u64)v >> 32), CTRL, 0xF, 0xF, true);
  return (long long)(((u64)hi << 32) | lo);
}
// The exact sum of one int32 of each of the 64 lanes, wave-uniform (all lanes call it): butterflies inside the quads
// (quad_perm [1,0,3,2], [2,3,0,1]), the half rows (row_half_mirror) and the rows (row_mirror) leave every lane with the sum of its
// row of 16; the four rows are added on the scalar side.
static __device__ __forceinline__ long long wave_sum_i64(int part)
{
  long long v = (long long)part;
  v += i64_dpp<0xB1>(v);
  v += i64_dpp<0x4E>(v);
  v += i64_dpp<0x141>(v);
  v += i64_dpp<0x140>(v);
  long long s = 0;
#pragma unroll
  for (int row = 0; row < 4; ++row) {
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, 16 * row), hi = (u32)__builtin_amdgcn_readlane((int)(u32)((u64)v >> 32), 16 * row);
    s += (long long)(((u64)hi << 32) | lo);
  }
  return s;
}
static __device__ __forceinline__ float f32_of_sum(long long s) { return (float)(double)s; }  // |s| < 2^53: one rounding

// a position of the window's corner: the integer part, tested as floats (NaN and values beyond int32 are out), and the weights
struct FlowPos { bool out; int ix, iy, w00, w01, w10, w11; };
static __device__ __forceinline__ FlowPos flow_pos(float qx, float qy, int win, int W, int H)
{
  FlowPos r{};
  const float fx = __builtin_floorf(qx), fy = __builtin_floorf(qy);
  r.out = !(fx >= (float)-win && fx < (float)W && fy >= (float)-win && fy < (float)H);
  if (r.out) return r;
  r.ix = (int)fx; r.iy = (int)fy;
  const float a = __fsub_rn(qx, fx), b = __fsub_rn(qy, fy);
  const float t0 = __fsub_rn(1.0f, a), t1 = __fsub_rn(1.0f, b);
  r.w00 = (int)__builtin_rintf(__fmul_rn(__fmul_rn(t0, t1), 16384.0f));
  r.w01 = (int)__builtin_rintf(__fmul_rn(__fmul_rn(a, t1), 16384.0f));
  r.w10 = (int)__builtin_rintf(__fmul_rn(__fmul_rn(t0, b), 16384.0f));
  r.w11 = 16384 - r.w00 - r.w01 - r.w10;
  return r;
}

template <int NR>
__global__ __launch_bounds__(64 * FLOW_WAVES) void k_lk_flow(const FlowParams p)
{
  const int lane = threadIdx.x & 63;
  const u32 slot = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * FLOW_WAVES + (threadIdx.x >> 6)));
  const int frame = blockIdx.y;
  if ((size_t)slot >= p.capacity || slot >= p.counts[frame]) return;  // wave-uniform
  const int W = p.W, H = p.H, win = p.win, ww = win * win, level = p.level;
  const size_t pi = (size_t)frame * p.capacity + slot;
  const u32 pbx = reinterpret_cast<const u32 *>(p.prev_pts)[2 * pi], pby = reinterpret_cast<const u32 *>(p.prev_pts)[2 * pi + 1];
  u32 sbx = pbx, sby = pby;  // the start, bit for bit: what a lost point is left with
  if (p.use_initial) { sbx = reinterpret_cast<const u32 *>(p.next_pts)[2 * pi]; sby = reinterpret_cast<const u32 *>(p.next_pts)[2 * pi + 1]; }
  const float s = __uint_as_float((u32)(127 - level) << 23), S = __uint_as_float((u32)(127 + level) << 23);  // 2^-level, 2^level
  const float hw = __fmul_rn((float)(win - 1), 0.5f);
  const uint8_t *const prev = p.prev + (size_t)frame * p.frame_stride, *const next = p.next + (size_t)frame * p.frame_stride;
  const u32 pitch = (u32)p.pitch;  // (H * pitch < 2^32)

  // the lane's pixels: TI[r] = I | i << 16 | j << 24, G[r] = (gx, gy) as an int16 pair; zeros for the idle ones
  u32 TI[NR], G[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) TI[r] = G[r] = 0;
  bool lost = false;
  float f11 = 0, f12 = 0, f22 = 0, Dinv = 0;
  {
    const FlowPos u = flow_pos(__fsub_rn(__fmul_rn(__uint_as_float(pbx), s), hw), __fsub_rn(__fmul_rn(__uint_as_float(pby), s), hw), win, W, H);
    lost = u.out;
    int a11 = 0, a12 = 0, a22 = 0;
    if (!lost) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int t = lane + 64 * r;
        if (t < ww) {
          const int j = t / win, i = t - j * win;
          int P[4][4];
          u32 xo[4], yo[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            xo[k] = (u32)min(max(u.ix + i - 1 + k, 0), W - 1);
            yo[k] = (u32)min(max(u.iy + j - 1 + k, 0), H - 1) * pitch;
          }
#pragma unroll
          for (int y = 0; y < 4; ++y)
#pragma unroll
            for (int x = 0; x < 4; ++x) P[y][x] = (int)prev[yo[y] + xo[x]];
          int dx[2][2], dy[2][2];
#pragma unroll
          for (int y = 1; y < 3; ++y)
#pragma unroll
            for (int x = 1; x < 3; ++x) {
              dx[y - 1][x - 1] = 3 * (P[y - 1][x + 1] - P[y - 1][x - 1]) + 10 * (P[y][x + 1] - P[y][x - 1]) + 3 * (P[y + 1][x + 1] - P[y + 1][x - 1]);
              dy[y - 1][x - 1] = 3 * (P[y + 1][x - 1] - P[y - 1][x - 1]) + 10 * (P[y + 1][x] - P[y - 1][x]) + 3 * (P[y + 1][x + 1] - P[y - 1][x + 1]);
            }
          const int iv = (u.w00 * P[1][1] + u.w01 * P[1][2] + u.w10 * P[2][1] + u.w11 * P[2][2] + 256) >> 9;
          const int gx = (u.w00 * dx[0][0] + u.w01 * dx[0][1] + u.w10 * dx[1][0] + u.w11 * dx[1][1] + 8192) >> 14;
          const int gy = (u.w00 * dy[0][0] + u.w01 * dy[0][1] + u.w10 * dy[1][0] + u.w11 * dy[1][1] + 8192) >> 14;
          TI[r] = ((u32)iv & 0xFFFFu) | ((u32)i << 16) | ((u32)j << 24);
          G[r] = ((u32)gx & 0xFFFFu) | ((u32)gy << 16);
          a11 += gx * gx; a12 += gx * gy; a22 += gy * gy;  // (|gx|, |gy| <= 4080, 16 rounds at most: below 2^29)
        }
      }
      const long long A11 = wave_sum_i64(a11), A12 = wave_sum_i64(a12), A22 = wave_sum_i64(a22);
      const float sc = 9.5367431640625e-07f;  // 2^-20
      f11 = __fmul_rn(f32_of_sum(A11), sc); f12 = __fmul_rn(f32_of_sum(A12), sc); f22 = __fmul_rn(f32_of_sum(A22), sc);
      const float D = __fsub_rn(__fmul_rn(f11, f22), __fmul_rn(f12, f12));
      const float d = __fsub_rn(f11, f22);
      const float m = __fsub_rn(__fadd_rn(f22, f11), __builtin_sqrtf(__fadd_rn(__fmul_rn(d, d), __fmul_rn(4.0f, __fmul_rn(f12, f12)))));
      const float min_eig = m / (float)(2 * ww);
      lost = min_eig < p.min_eig || D < 1.1920929e-7f;
      Dinv = 1.0f / D;
    }
  }

  // diff of the lane's pixel of round r at a position (the pixel is not idle); all fetches clamped
  auto diff_at = [&](const FlowPos &q, u32 ti) -> int {
    const int x = q.ix + (int)((ti >> 16) & 0xFFu), y = q.iy + (int)(ti >> 24);
    const u32 x0 = (u32)min(max(x, 0), W - 1), x1 = (u32)min(max(x + 1, 0), W - 1);
    const u32 y0 = (u32)min(max(y, 0), H - 1) * pitch, y1 = (u32)min(max(y + 1, 0), H - 1) * pitch;
    const int v = (q.w00 * (int)next[y0 + x0] + q.w01 * (int)next[y0 + x1] + q.w10 * (int)next[y1 + x0] + q.w11 * (int)next[y1 + x1] + 256) >> 9;
    return v - (int)(short)(ti & 0xFFFFu);
  };

  float vx = __fsub_rn(__fmul_rn(__uint_as_float(sbx), s), hw), vy = __fsub_rn(__fmul_rn(__uint_as_float(sby), s), hw);
  if (!lost) {
    float px = 0.0f, py = 0.0f;
#pragma nounroll
    for (int k = 0; k < p.max_iterations; ++k) {  // everything but the pixel sums is wave-uniform
      const FlowPos q = flow_pos(vx, vy, win, W, H);
      if (q.out) { lost = true; break; }
      int b1 = 0, b2 = 0;
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (lane + 64 * r < ww) {
          const int df = diff_at(q, TI[r]);
          b1 += df * (int)(short)(G[r] & 0xFFFFu);  // (|df| <= 8162, |g| <= 4080, 16 rounds at most: below 2^30)
          b2 += df * ((int)G[r] >> 16);
        }
      const long long B1 = wave_sum_i64(b1), B2 = wave_sum_i64(b2);
      const float sc = 9.5367431640625e-07f;
      const float g1 = __fmul_rn(f32_of_sum(B1), sc), g2 = __fmul_rn(f32_of_sum(B2), sc);
      const float ex = __fmul_rn(__fsub_rn(__fmul_rn(f12, g2), __fmul_rn(f22, g1)), Dinv);
      const float ey = __fmul_rn(__fsub_rn(__fmul_rn(f12, g1), __fmul_rn(f11, g2)), Dinv);
      vx = __fadd_rn(vx, ex); vy = __fadd_rn(vy, ey);
      if (__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)) <= p.eps2) break;
      if (k > 0 && __builtin_fabsf(__fadd_rn(ex, px)) < 0.01f && __builtin_fabsf(__fadd_rn(ey, py)) < 0.01f) {
        vx = __fsub_rn(vx, __fmul_rn(ex, 0.5f)); vy = __fsub_rn(vy, __fmul_rn(ey, 0.5f));
        break;
      }
      px = ex; py = ey;
    }
  }

  u32 ox = sbx, oy = sby;
  if (!lost) { ox = __float_as_uint(__fmul_rn(__fadd_rn(vx, hw), S)); oy = __float_as_uint(__fmul_rn(__fadd_rn(vy, hw), S)); }
  if (lane == 0) { reinterpret_cast<u32 *>(p.next_pts)[2 * pi] = ox; reinterpret_cast<u32 *>(p.next_pts)[2 * pi + 1] = oy; }
  if (level != 0) return;
  FlowPos q{};
  q.out = true;
  if (!lost) q = flow_pos(vx, vy, win, W, H);
  const bool ok = !q.out;  // wave-uniform
  float err = 0.0f;
  if (p.err && ok) {
    int e = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (lane + 64 * r < ww) e += abs(diff_at(q, TI[r]));
    err = f32_of_sum(wave_sum_i64(e)) / (float)(32 * ww);
  }
  if (lane == 0) {
    p.status[pi] = ok ? 1 : 0;
    if (p.err) p.err[pi] = err;
  }
}

}  // namespace

hipError_t launch_pyr_down(const PyrParams &p, hipStream_t s)
{
  if (p.W < PYR_MIN_SIDE || p.H < PYR_MIN_SIDE || p.dW != pyr_half(p.W) || p.dH != pyr_half(p.H) || p.nframes < 1 || !p.in || !p.out || p.in_pitch < (size_t)p.W
      || p.out_pitch < (size_t)p.dW || p.in_pitch > 0xFFFFFFFFull / (size_t)p.H || p.out_pitch > 0xFFFFFFFFull / (size_t)p.dH
      || (p.in_aligned && (((uintptr_t)p.in | p.in_pitch | p.in_frame_stride) & 3u)) || (p.out_aligned && (((uintptr_t)p.out | p.out_pitch | p.out_frame_stride) & 1u))
      || p.nstrips != pyr_strips(p.W) || p.nchunks != pyr_chunks(p.dH) || (long long)p.total_items != (long long)p.nframes * p.nstrips * p.nchunks)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pyr_down8, dim3((p.total_items + 3) / 4), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_lk_flow(const FlowParams &p, hipStream_t s)
{
  if (p.W < 1 || p.H < 1 || p.nframes < 1 || p.nframes > 65535 || !p.prev || !p.next || !p.counts || !p.prev_pts || !p.next_pts || !p.status || p.pitch < (size_t)p.W
      || p.pitch > 0xFFFFFFFFull / (size_t)p.H || !flow_win_ok(p.win) || p.level < 0 || p.level > FLOW_MAX_LEVEL || p.max_iterations < 1
      || p.max_iterations > FLOW_MAX_ITERATIONS || p.capacity < 1 || (size_t)p.groups != (p.capacity + FLOW_WAVES - 1) / FLOW_WAVES
      || (((uintptr_t)p.counts | (uintptr_t)p.prev_pts | (uintptr_t)p.next_pts | (uintptr_t)p.err) & 3u) || !(p.eps2 >= 0) || !(p.min_eig >= 0))
    return hipErrorInvalidValue;
  const dim3 grid(p.groups, (unsigned)p.nframes), block(64 * FLOW_WAVES);
  switch (flow_round_class(p.win)) {
  case 1: hipLaunchKernelGGL(k_lk_flow<1>, grid, block, 0, s, p); break;
  case 2: hipLaunchKernelGGL(k_lk_flow<2>, grid, block, 0, s, p); break;
  case 4: hipLaunchKernelGGL(k_lk_flow<4>, grid, block, 0, s, p); break;
  case 7: hipLaunchKernelGGL(k_lk_flow<7>, grid, block, 0, s, p); break;
  case 10: hipLaunchKernelGGL(k_lk_flow<10>, grid, block, 0, s, p); break;
  default: hipLaunchKernelGGL(k_lk_flow<16>, grid, block, 0, s, p); break;
  }
  return hipGetLastError();
}

}  // namespace hc
