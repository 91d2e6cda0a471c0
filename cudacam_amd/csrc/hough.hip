// hough.hip -- cv::HoughLines' standard transform (srn = stn = 0) from the point lists of hc_edge_points_device, per frame
// (hc_hough_lines_device; the contract is stated in include/hipcanny.h and restated in tests/hough_ref.py).
//
//   k_hough_vote   a workgroup is (frame, group of `rows` consecutive angles).  It keeps the group's accumulator rows in LDS
//                  (dynamic, up to all 160 KiB of a CU), zeroes them, streams the frame's point list -- one 8-byte load per lane,
//                  consecutive lanes consecutive points -- and adds one vote per point and angle with an LDS atomic whose
//                  result nobody reads (ds_add_u32).  Then it stores its rows whole, zeros included, so the accumulator needs
//                  no memset; the first and the last group of a frame also store the two padding rows.  No global atomics:
//                  a row belongs to one workgroup, and the sums are integers, so the order of the waves changes nothing.
//   k_hough_peaks  a work item is (frame, angle row) and belongs to one wave, which walks the row in trips of 64 cells and
//                  applies the peak rule.  <false>: the row's number of peaks -> items[frame][row].  <true>: the peaks as
//                  (votes, accumulator index) pairs from the row's offset on, in index order (ballot + v_mbcnt, as k_edge_emit).
//   k_hough_scan   one wave per frame: exclusive prefix sum over the frame's rows in place, the total -> line_counts[frame].
//   k_hough_rank   a lane per peak: it counts the peaks that precede its own in the order (votes descending, index ascending),
//                  the frame's list passing through LDS in tiles of 256, and writes its line at that rank if the rank is below
//                  line_capacity.  The keys are unique, so the ranks are a permutation: no two lanes write one line.
//                  Quadratic in the peaks of a frame; not launched when line_capacity == 0.
//
// The vote: r = rint(x * tab_cos[n] + y * tab_sin[n]) in float32 -- two rounded products and one rounded sum, no FMA (this
// file is compiled with -ffp-contract=off, and says so itself below).  The bound test is made on the rounded FLOAT, before any
// conversion: a coordinate of any size, an infinite or a NaN sum fails it and votes nowhere, so no LDS word outside the row is
// ever addressed.
#include "canny_device.h"

#pragma clang fp contract(off)

namespace hc {

namespace {

__global__ __launch_bounds__(HOUGH_VOTE_THREADS) void k_hough_vote(const HoughParams p)
{
  extern __shared__ u32 hough_rows[];  // [na][numrho + 2]
  const int frame = (int)blockIdx.x / p.groups, group = (int)blockIdx.x % p.groups;
  const int n0 = group * p.rows, na = min(p.rows, p.numangle - n0);
  const int stride = p.numrho + 2, words = na * stride;  // (words * 4 <= HOUGH_LDS_BYTES)
  for (int i = threadIdx.x; i < words; i += HOUGH_VOTE_THREADS) hough_rows[i] = 0u;
  float tc[HOUGH_MAX_ROWS], ts[HOUGH_MAX_ROWS];
#pragma unroll
  for (int a = 0; a < HOUGH_MAX_ROWS; ++a) {
    tc[a] = a < na ? p.tab_cos[n0 + a] : 0.0f;
    ts[a] = a < na ? p.tab_sin[n0 + a] : 0.0f;
  }
  __syncthreads();
  const size_t npts = min((size_t)p.point_counts[frame], p.point_capacity);
  const int2 *pts = reinterpret_cast<const int2 *>(p.points) + (size_t)frame * p.point_capacity;
  const int half = (p.numrho - 1) / 2;
  const float lo = (float)(-1 - half), hi = (float)(p.numrho - half);  // r + half in -1 .. numrho; both exact in float
  for (size_t i = threadIdx.x; i < npts; i += HOUGH_VOTE_THREADS) {
    const int2 q = pts[i];
    const float x = (float)q.x, y = (float)q.y;
#pragma unroll
    for (int a = 0; a < HOUGH_MAX_ROWS; ++a)
      if (a < na) {
        const float rf = rintf(__fadd_rn(__fmul_rn(x, tc[a]), __fmul_rn(y, ts[a])));
        if (rf >= lo && rf <= hi) atomicAdd(&hough_rows[a * stride + ((int)rf + half + 1)], 1u);
      }
  }
  __syncthreads();
  u32 *acc = reinterpret_cast<u32 *>(p.accum) + (size_t)frame * (size_t)(p.numangle + 2) * (size_t)stride;
  u32 *dst = acc + (size_t)(n0 + 1) * (size_t)stride;
  for (int i = threadIdx.x; i < words; i += HOUGH_VOTE_THREADS) dst[i] = hough_rows[i];
  if (group == 0)
    for (int i = threadIdx.x; i < stride; i += HOUGH_VOTE_THREADS) acc[i] = 0u;
  if (group == p.groups - 1) {
    u32 *last = acc + (size_t)(p.numangle + 1) * (size_t)stride;
    for (int i = threadIdx.x; i < stride; i += HOUGH_VOTE_THREADS) last[i] = 0u;
  }
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_hough_peaks(const HoughParams p)
{
  const int lane = threadIdx.x & 63;
  const int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (item >= p.nframes * p.numangle) return;
  const int frame = item / p.numangle, n = item % p.numangle;
  const int stride = p.numrho + 2;
  const int32_t *mid = p.accum + (size_t)frame * (size_t)(p.numangle + 2) * (size_t)stride + (size_t)(n + 1) * (size_t)stride;
  const int32_t *up = mid - stride, *down = mid + stride;  // (rows n and n + 2 of the padded accumulator)
  uint2 *out = reinterpret_cast<uint2 *>(p.peaks) + (size_t)frame * p.peak_cap;
  u32 off = EMIT ? (u32)__builtin_amdgcn_readfirstlane((int)p.items[item]) : 0u;  // wave-uniform: index of the row's next peak / its count
  for (int r0 = 0; r0 < p.numrho; r0 += 64) {
    const int r = r0 + lane;
    int a = 0;
    bool pk = false;
    if (r < p.numrho) {
      a = mid[r + 1];
      pk = a > p.threshold && a > mid[r] && a >= mid[r + 2] && a > up[r + 1] && a >= down[r + 1];
    }
    const u64 m = __ballot(pk);
    if (EMIT && pk) {
      const size_t slot = (size_t)off + mbcnt64(m);
      if (slot < p.peak_cap) out[slot] = make_uint2((u32)a, (u32)((n + 1) * stride + r + 1));
    }
    off += (u32)__popcll(m);
  }
  if (!EMIT && lane == 0) p.items[item] = off;
}

__global__ __launch_bounds__(256) void k_hough_scan(const HoughParams p)
{
  const int lane = threadIdx.x & 63;
  const int frame = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (frame >= p.nframes) return;
  u32 *it = p.items + (size_t)frame * p.numangle;
  u32 carry = 0;  // (a frame has fewer than 2^30 peaks: half its cells at most)
  for (int c0 = 0; c0 < p.numangle; c0 += 64) {
    const int c = c0 + lane;
    const u32 v = c < p.numangle ? it[c] : 0u;
    u32 incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (c < p.numangle) it[c] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
  if (lane == 0) p.line_counts[frame] = carry;
}

__global__ __launch_bounds__(HOUGH_RANK_THREADS) void k_hough_rank(const HoughParams p)
{
  __shared__ uint2 tile[HOUGH_RANK_THREADS];
  const int frame = blockIdx.y;
  const u32 np = (u32)min((size_t)p.line_counts[frame], p.peak_cap);  // uniform in the workgroup
  const u32 i0 = blockIdx.x * HOUGH_RANK_THREADS;
  if (i0 >= np) return;
  const uint2 *pk = reinterpret_cast<const uint2 *>(p.peaks) + (size_t)frame * p.peak_cap;
  const u32 i = i0 + threadIdx.x;
  const uint2 me = i < np ? pk[i] : make_uint2(0u, 0u);
  const u32 rank = peak_rank(pk, np, me, tile);
  if (i >= np || (size_t)rank >= p.line_capacity) return;
  const int stride = p.numrho + 2;
  const int n = (int)(me.y / (u32)stride) - 1, r = (int)(me.y % (u32)stride) - 1;
  float *o = p.lines + ((size_t)frame * p.line_capacity + rank) * 3;
  o[0] = __fmul_rn(__fsub_rn((float)r, __fmul_rn((float)(p.numrho - 1), 0.5f)), p.rho);
  o[1] = p.tab_theta[n];
  o[2] = (float)me.x;
}

}  // namespace

// what k_hough_peaks and k_hough_scan need of a block: the accumulator, the peak list and the per-row counts of one pass
static bool peaks_ok(const HoughParams &p)
{
  const long long stride = (long long)p.numrho + 2, cells = ((long long)p.numangle + 2) * stride;
  return p.accum && p.items && p.peaks && p.line_counts && !((((uintptr_t)p.line_counts | (uintptr_t)p.accum | (uintptr_t)p.items) & 3u) | ((uintptr_t)p.peaks & 7u))
         && p.numangle >= 1 && p.numrho >= 0 && p.nframes >= 1 && p.threshold >= 0 && cells < (1ll << 31) && (long long)p.nframes * p.numangle <= 0x7FFFFFF0ll
         && p.peak_cap == (size_t)p.numangle * (size_t)((p.numrho + 1) / 2);
}

// The peaks of the padded accumulators p.accum [nframes][numangle + 2][numrho + 2] on stream s: count, scan (the frames' totals ->
// p.line_counts) and, where a cell can be a peak at all, emit.  Of p it reads accum, items, peaks, peak_cap, line_counts, numangle,
// numrho, nframes and threshold only: hc_hough_circles_device calls it on its own accumulator (rows = numangle, columns = numrho).
hipError_t launch_hough_peaks(const HoughParams &p, hipStream_t s)
{
  if (!peaks_ok(p)) return hipErrorInvalidValue;
  const dim3 rows_grid((unsigned)(((long long)p.nframes * p.numangle + 3) / 4)), block(256);
  hipLaunchKernelGGL(k_hough_peaks<false>, rows_grid, block, 0, s, p);
  hipLaunchKernelGGL(k_hough_scan, dim3((p.nframes + 3) / 4), block, 0, s, p);
  if (p.peak_cap) hipLaunchKernelGGL(k_hough_peaks<true>, rows_grid, block, 0, s, p);
  return hipGetLastError();
}

// One pass on stream s: the votes, the peaks (count, scan, emit) and, with p.line_capacity > 0, the ranking.
hipError_t launch_hough(const HoughParams &p, hipStream_t s)
{
  const long long stride = (long long)p.numrho + 2;
  if (!peaks_ok(p) || !p.points || !p.point_counts || !p.tab_cos || !p.tab_sin || !p.tab_theta || (((uintptr_t)p.points & 7u) | (((uintptr_t)p.point_counts | (uintptr_t)p.lines) & 3u))
      || (p.line_capacity && !p.lines) || p.rows < 1 || p.rows > HOUGH_MAX_ROWS || (long long)p.rows * stride * 4 > HOUGH_LDS_BYTES || p.groups != (p.numangle + p.rows - 1) / p.rows
      || (long long)p.nframes * p.groups > 0x7FFFFFF0ll || p.nframes > 65535)
    return hipErrorInvalidValue;
  const size_t lds = (size_t)p.rows * (size_t)stride * 4;
  if (lds > 64 * 1024) {  // above the default bound of dynamic LDS the kernel has to be told
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_hough_vote), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_hough_vote, dim3((unsigned)(p.nframes * p.groups)), dim3(HOUGH_VOTE_THREADS), lds, s, p);
  if (const hipError_t e = launch_hough_peaks(p, s)) return e;
  if (p.peak_cap && p.line_capacity)
    hipLaunchKernelGGL(k_hough_rank, dim3((unsigned)((p.peak_cap + HOUGH_RANK_THREADS - 1) / HOUGH_RANK_THREADS), (unsigned)p.nframes), dim3(HOUGH_RANK_THREADS), 0, s, p);
  return hipGetLastError();
}

}  // namespace hc
