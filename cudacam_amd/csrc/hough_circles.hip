// hough_circles.hip -- circles from the point lists of hc_edge_points_device and the int16 gradient planes of hc_derivatives_device,
// per frame: centres voted along the gradient, sifted by a smallest distance, and a radius histogram for each kept centre
// (hc_hough_circles_device: the form of cv::cuda::HoughCirclesDetector; the contract is stated in include/hipcanny.h and restated
// in tests/hough_circles_ref.py).
//
//   k_circle_vote   a lane per point, one 8-byte load per lane.  A point inside the frame reads its two gradients and walks the ray
//                   through it in both directions, radius by radius, in Q10 fixed point; every cell it reaches gets one vote: a
//                   global atomic add whose result nobody reads.  A 1080p accumulator is 8.3 MB and fits no LDS.  The votes are
//                   integer sums: the accumulator is a function of the input alone, whatever the order.  The accumulator is zeroed
//                   before the launch, on the same stream.
//   the peaks       k_hough_peaks and k_hough_scan of hough.hip on this accumulator (launch_hough_peaks): same padding, same rule.
//   k_circle_rank   the comparison loop of k_hough_rank (peak_rank, canny_device.h): a lane per peak; ranks below centre_capacity
//                   write (votes, cx, cy) into the ranked list.
//   k_circle_sift   one wave per frame goes through the ranked centres in order; the kept list sits in LDS (8 bytes a centre) and
//                   the lanes compare the candidate with 64 kept centres per trip (sift_min_distance, canny_device.h).
//   k_circle_radii  a workgroup per (frame, kept-centre slot): the histogram of the distances of the frame's points from the
//                   centre, in LDS with LDS atomics whose result nobody reads, then the radius rule by the workgroup's first wave,
//                   64 radii per trip.  <false>: the centre's circle count -> items.  <true>: the histogram again, and the circles
//                   from the centre's offset on in ascending radius (ballot + v_mbcnt, as k_edge_emit); no atomics on the output.
//   k_circle_scan   one wave per frame: exclusive prefix sum over the frame's kept centres in place, the total -> circle_counts.
//
// Every float step of the contract is one rounded float32 operation (__fmul_rn and its kin; this file is compiled with
// -ffp-contract=off, and says so itself below).  A point is tested against the frame before any address is formed from it; a walk
// tests its cell against the accumulator before it forms the cell's address.
#include "canny_device.h"

#pragma clang fp contract(off)

namespace hc {

namespace {

static __device__ __forceinline__ bool in_frame(int2 q, int W, int H) { return (u32)q.x < (u32)W && (u32)q.y < (u32)H; }

__global__ __launch_bounds__(CIRCLE_THREADS) void k_circle_vote(const CircleParams p)
{
  const int frame = blockIdx.y;
  const size_t npts = min((size_t)p.point_counts[frame], p.point_capacity);
  const int2 *pts = reinterpret_cast<const int2 *>(p.points) + (size_t)frame * p.point_capacity;
  const char *gx = reinterpret_cast<const char *>(p.dx) + (size_t)frame * p.frame_stride;
  const char *gy = reinterpret_cast<const char *>(p.dy) + (size_t)frame * p.frame_stride;
  const int stride = p.AW + 2;
  int32_t *acc = p.accum + (size_t)frame * (size_t)(p.AH + 2) * (size_t)stride;
  for (size_t i = (size_t)blockIdx.x * CIRCLE_THREADS + threadIdx.x; i < npts; i += (size_t)gridDim.x * CIRCLE_THREADS) {
    const int2 q = pts[i];
    if (!in_frame(q, p.W, p.H)) continue;
    const size_t at = (size_t)q.y * p.pitch + 2 * (size_t)q.x;  // (H * pitch < 2^32)
    const int vx = *reinterpret_cast<const int16_t *>(gx + at), vy = *reinterpret_cast<const int16_t *>(gy + at);
    if (vx == 0 && vy == 0) continue;
    const float mag = __fsqrt_rn((float)((u32)(vx * vx) + (u32)(vy * vy)));  // (at most 2^31: exact in uint32)
    const int x0 = (int)rintf(__fmul_rn(__fmul_rn((float)q.x, p.idp), 1024.0f)), y0 = (int)rintf(__fmul_rn(__fmul_rn((float)q.y, p.idp), 1024.0f));
    const int sx = (int)rintf(__fdiv_rn(__fmul_rn(__fmul_rn((float)vx, p.idp), 1024.0f), mag));
    const int sy = (int)rintf(__fdiv_rn(__fmul_rn(__fmul_rn((float)vy, p.idp), 1024.0f), mag));
#pragma unroll
    for (int d = 1; d >= -1; d -= 2) {
      int x1 = x0 + d * p.min_radius * sx, y1 = y0 + d * p.min_radius * sy;  // (|x0| <= 2^30, |min_radius * sx| < 2^30)
      for (int r = p.min_radius; r <= p.max_radius; ++r) {
        const int x2 = x1 >> 10, y2 = y1 >> 10;
        if ((u32)x2 >= (u32)p.AW || (u32)y2 >= (u32)p.AH) break;
        atomicAdd(&acc[(y2 + 1) * stride + x2 + 1], 1);
        x1 += d * sx;
        y1 += d * sy;
      }
    }
  }
}

__global__ __launch_bounds__(HOUGH_RANK_THREADS) void k_circle_rank(const CircleParams p)
{
  __shared__ uint2 tile[HOUGH_RANK_THREADS];
  const int frame = blockIdx.y;
  const u32 np = (u32)min((size_t)p.npeaks[frame], p.peak_cap);  // uniform in the workgroup
  const u32 i0 = blockIdx.x * HOUGH_RANK_THREADS;
  if (i0 >= np) return;
  const uint2 *pk = reinterpret_cast<const uint2 *>(p.peaks) + (size_t)frame * p.peak_cap;
  const u32 i = i0 + threadIdx.x;
  const uint2 me = i < np ? pk[i] : make_uint2(0u, 0u);
  const u32 rank = peak_rank(pk, np, me, tile);
  if (i >= np || rank >= (u32)p.centre_capacity) return;
  const u32 stride = (u32)p.AW + 2;
  reinterpret_cast<int4 *>(p.ranked)[(size_t)frame * p.centre_capacity + rank] = make_int4((int)me.x, (int)(me.y % stride) - 1, (int)(me.y / stride) - 1, 0);
}

__global__ __launch_bounds__(64) void k_circle_sift(const CircleParams p)
{
  __shared__ int2 kept_xy[CIRCLE_MAX_CENTRES];
  const int lane = threadIdx.x;
  const int frame = blockIdx.x;
  const u32 nc = min(p.npeaks[frame], (u32)p.centre_capacity);
  const int4 *in = reinterpret_cast<const int4 *>(p.ranked) + (size_t)frame * p.centre_capacity;
  int4 *out = reinterpret_cast<int4 *>(p.kept) + (size_t)frame * p.centre_capacity;
  const u32 nk = sift_min_distance(in, nc, p.min_d2, kept_xy, out);  // (canny_device.h: shared with k_feat_sift)
  if (lane == 0) p.nkept[frame] = nk;
}

template <bool EMIT>
__global__ __launch_bounds__(CIRCLE_THREADS) void k_circle_radii(const CircleParams p)
{
  __shared__ u32 hist[CIRCLE_MAX_HIST];
  const int frame = blockIdx.y;
  const u32 slot = blockIdx.x;
  if (slot >= p.nkept[frame]) return;  // (k_circle_scan reads the kept slots only)
  const int nr = p.max_radius - p.min_radius + 1, words = nr + 2;  // hist[i + 1] counts radius min_radius + i; both ends stay zero
  for (int i = threadIdx.x; i < words; i += CIRCLE_THREADS) hist[i] = 0u;
  __syncthreads();
  const int4 ctr = reinterpret_cast<const int4 *>(p.kept)[(size_t)frame * p.centre_capacity + slot];
  const float fx = __fmul_rn(__fadd_rn((float)ctr.y, 0.5f), p.dp), fy = __fmul_rn(__fadd_rn((float)ctr.z, 0.5f), p.dp);
  const float rmin = (float)p.min_radius, rmax = (float)p.max_radius;
  const size_t npts = min((size_t)p.point_counts[frame], p.point_capacity);
  const int2 *pts = reinterpret_cast<const int2 *>(p.points) + (size_t)frame * p.point_capacity;
  for (size_t i = threadIdx.x; i < npts; i += CIRCLE_THREADS) {
    const int2 q = pts[i];
    if (!in_frame(q, p.W, p.H)) continue;
    const float ddx = __fsub_rn(fx, (float)q.x), ddy = __fsub_rn(fy, (float)q.y);
    const float rad = __fsqrt_rn(__fadd_rn(__fmul_rn(ddx, ddx), __fmul_rn(ddy, ddy)));
    if (rad >= rmin && rad <= rmax) atomicAdd(&hist[(int)rintf(__fsub_rn(rad, rmin)) + 1], 1u);  // (0 <= rad - rmin <= nr - 1)
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  const size_t item = (size_t)frame * p.centre_capacity + slot;
  u32 off = EMIT ? (u32)__builtin_amdgcn_readfirstlane((int)p.items[item]) : 0u;  // wave-uniform: index of the centre's next circle / its count
  const u32 cap = (u32)min(p.circle_capacity, (size_t)0xFFFFFFFFu);
  float4 *out = reinterpret_cast<float4 *>(p.circles) + (size_t)frame * p.circle_capacity;
  for (int i0 = 0; i0 < nr && (!EMIT || off < cap); i0 += 64) {
    const int i = i0 + lane;
    u32 h = 0;
    bool is = false;
    if (i < nr) {
      h = hist[i + 1];
      is = h >= (u32)p.threshold && h > hist[i] && h >= hist[i + 2];
    }
    const u64 m = __ballot(is);
    if (EMIT && is) {
      const u32 at = off + mbcnt64(m);
      if (at < cap) out[at] = make_float4(fx, fy, (float)(i + p.min_radius), (float)h);
    }
    off += (u32)__popcll(m);
  }
  if (!EMIT && lane == 0) p.items[item] = off;
}

__global__ __launch_bounds__(256) void k_circle_scan(const CircleParams p)
{
  const int lane = threadIdx.x & 63;
  const int frame = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (frame >= p.nframes) return;
  u32 *it = p.items + (size_t)frame * p.centre_capacity;
  const u32 nk = p.nkept[frame];
  u32 carry = 0;  // (a frame has fewer than 2^32 circles: 4096 centres of fewer than 4096 radii)
  for (u32 c0 = 0; c0 < nk; c0 += 64) {
    const u32 c = c0 + lane;
    const u32 v = c < nk ? it[c] : 0u;
    u32 incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (c < nk) it[c] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
  if (lane == 0) p.circle_counts[frame] = carry;
}

}  // namespace

// One pass on stream s, behind the zeroing of p.accum.  circle_capacity == 0: counts only (k_circle_radii<true> is not launched,
// p.circles is not looked at).
hipError_t launch_hough_circles(const CircleParams &p, hipStream_t s)
{
  const long long cells = ((long long)p.AH + 2) * ((long long)p.AW + 2);
  if (!p.points || !p.point_counts || !p.dx || !p.dy || !p.accum || !p.row_items || !p.peaks || !p.npeaks || !p.ranked || !p.kept || !p.nkept || !p.items || !p.circle_counts
      || (((uintptr_t)p.points | (uintptr_t)p.peaks) & 7u) || (((uintptr_t)p.ranked | (uintptr_t)p.kept) & 15u)
      || (((uintptr_t)p.point_counts | (uintptr_t)p.accum | (uintptr_t)p.row_items | (uintptr_t)p.npeaks | (uintptr_t)p.nkept | (uintptr_t)p.items | (uintptr_t)p.circle_counts) & 3u)
      || (((uintptr_t)p.dx | (uintptr_t)p.dy | p.pitch | p.frame_stride) & 1u) || p.W < 1 || p.H < 1 || p.AW < 1 || p.AH < 1 || p.AW > p.W || p.AH > p.H || cells >= (1ll << 31)
      || p.pitch < 2 * (size_t)p.W || (unsigned long long)p.H * p.pitch >= (1ull << 32) || p.nframes < 1 || p.nframes > 65535 || p.centre_capacity < 1
      || p.centre_capacity > CIRCLE_MAX_CENTRES || p.threshold < 0 || p.min_radius < 1 || p.max_radius < p.min_radius || p.max_radius - p.min_radius + 3 > CIRCLE_MAX_HIST
      || (long long)p.W + p.max_radius >= (1 << 20) || (long long)p.H + p.max_radius >= (1 << 20) || !(p.idp > 0.0f) || !(p.idp <= 1.0f) || p.min_d2 < 0
      || p.vote_groups < 1 || p.vote_groups > (unsigned)CIRCLE_VOTE_GROUPS || p.rank_groups != (unsigned)((p.peak_cap + HOUGH_RANK_THREADS - 1) / HOUGH_RANK_THREADS) || p.peak_cap != (size_t)p.AH * (size_t)((p.AW + 1) / 2)
      || (p.circle_capacity && (!p.circles || ((uintptr_t)p.circles & 15u))))
    return hipErrorInvalidValue;
  HoughParams pk{};  // the accumulator as k_hough_peaks sees it: rows = AH, columns = AW
  pk.accum = p.accum; pk.items = p.row_items; pk.peaks = p.peaks; pk.peak_cap = p.peak_cap; pk.line_counts = p.npeaks;
  pk.numangle = p.AH; pk.numrho = p.AW; pk.nframes = p.nframes; pk.threshold = p.threshold;
  const unsigned n = (unsigned)p.nframes;
  hipLaunchKernelGGL(k_circle_vote, dim3(p.vote_groups, n), dim3(CIRCLE_THREADS), 0, s, p);
  if (const hipError_t e = launch_hough_peaks(pk, s)) return e;
  hipLaunchKernelGGL(k_circle_rank, dim3(p.rank_groups, n), dim3(HOUGH_RANK_THREADS), 0, s, p);
  hipLaunchKernelGGL(k_circle_sift, dim3(n), dim3(64), 0, s, p);
  hipLaunchKernelGGL(k_circle_radii<false>, dim3((unsigned)p.centre_capacity, n), dim3(CIRCLE_THREADS), 0, s, p);
  hipLaunchKernelGGL(k_circle_scan, dim3((n + 3) / 4), dim3(256), 0, s, p);
  if (p.circle_capacity) hipLaunchKernelGGL(k_circle_radii<true>, dim3((unsigned)p.centre_capacity, n), dim3(CIRCLE_THREADS), 0, s, p);
  return hipGetLastError();
}

}  // namespace hc
