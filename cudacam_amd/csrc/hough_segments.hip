// hough_segments.hip -- the lines of hc_hough_lines_device walked over the edge maps and cut into segments by a largest gap and
// a smallest length, per frame (hc_hough_segments_device: the form of cv::cuda::HoughSegmentDetector; the contract is stated in
// include/hipcanny.h and restated in tests/hough_segments_ref.py).
//
//   k_seg_count  a work item is (frame, line slot) and belongs to one wave.  It finds the line's angle index by a binary search
//                of tab_theta (the lines carry copies of the table's entries: the match is bit for bit, or the line yields
//                nothing), then walks the line in chunks of 64 steps, one step per lane: the lane computes its sample, loads
//                the map byte, and a ballot gives the chunk's edge mask.  Four chunks are loaded together and skipped together
//                when all are empty.  The number of kept segments -> items[frame][line].
//   k_seg_scan   one wave per frame: exclusive prefix sum over the frame's lines in place, the total -> seg_counts[frame].
//   k_seg_emit   the same walk: a kept segment goes to the line's offset + the segments kept so far + v_mbcnt over the chunk's
//                kept flags, while that index is below seg_capacity.  Not launched when seg_capacity == 0.
//
// Groups.  An edge lane looks for the edge step before its own: the highest set bit of the edge mask below the lane, or the
// last edge step of the chunks before (prev_t, wave-uniform: it comes from ballots).  It starts a group when there is none or
// when more than max_gap steps lie between; the ballot of that is the start mask.  A starting lane with a step before it
// closes the group that ends there: the group began at the highest start flag below the lane, or at the carried start_t.  Both
// ends are step numbers, and a sample is a pure function of its step, so the end points are computed again and nothing moves
// between lanes.  The group still open after the last chunk is closed by the wave as a whole.  Groups close in ascending step
// order along the lanes and the chunks: the order of the output.
//
// The sample: m = rint((float)t * slope + line_rho * scale) in float32 -- two rounded products and one rounded sum, no FMA
// (this file is compiled with -ffp-contract=off, and says so itself below).  The range test is made on the rounded FLOAT before
// any conversion: a rho of any size, an infinite or a NaN sum fails it and addresses nothing.  A y-major walk touches one cache
// line per lane; that belongs to the algorithm.
#include "canny_device.h"

#pragma clang fp contract(off)

namespace hc {

namespace {

// the walk of one line: what the wave needs to turn a step into a pixel
struct SegWalk {
  const uint8_t *fbase;  // the frame's map
  u32 pitch;             // (height * pitch < 2^32)
  int major, L, M;       // 0: step = column, 1: step = row; steps; samples m in 0 .. M - 1
  float slope, c0;       // m = rint((float)t * slope + c0), c0 = line_rho * scale

  // step t's sample; false: it lies outside the frame (the float is tested: below 2^31 it converts, and m <= M - 1 is exact)
  __device__ __forceinline__ bool sample(int t, int &m) const
  {
    const float mf = rintf(__fadd_rn(__fmul_rn((float)t, slope), c0));
    if (!(mf >= 0.0f && mf <= 2147483520.0f)) return false;
    m = (int)mf;
    return m < M;
  }
  __device__ __forceinline__ bool edge(int t) const
  {
    int m = 0;
    if (t >= L || !sample(t, m)) return false;
    return fbase[major ? (u32)t * pitch + (u32)m : (u32)m * pitch + (u32)t] != 0;
  }
  // the group of edge steps first .. last (both are edges): its segment, and whether min_length keeps it
  __device__ __forceinline__ bool close(int first, int last, int min_length, int4 &seg) const
  {
    int m0 = 0, m1 = 0;
    (void)sample(first, m0);
    (void)sample(last, m1);
    seg = major ? make_int4(m0, first, m1, last) : make_int4(first, m0, last, m1);
    const long long dx = (long long)seg.z - seg.x, dy = (long long)seg.w - seg.y;
    return dx * dx + dy * dy >= (long long)min_length * min_length;
  }
};

template <bool EMIT>
static __device__ __forceinline__ void seg_walk(const SegParams &p)
{
  const int lane = threadIdx.x & 63;
  const int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (item >= p.total_items) return;
  const int frame = (int)((size_t)item / p.line_capacity);
  const size_t line = (size_t)item % p.line_capacity;
  if (line >= min((size_t)p.line_counts[frame], p.line_capacity)) return;  // (k_seg_scan reads the walked slots only)
  const float *ln = p.lines + (size_t)item * 3;
  const float line_rho = ln[0], line_theta = ln[1];
  int lo = 0, hi = p.numangle;  // the first entry not below the line's theta: tab_theta never descends
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (p.tab_theta[mid] < line_theta) lo = mid + 1;
    else hi = mid;
  }
  const int n = lo;
  u32 off = 0;  // EMIT: index of the line's next segment in the frame's list; otherwise the segments kept so far.  Wave-uniform.
  if (n < p.numangle && __float_as_uint(p.tab_theta[n]) == __float_as_uint(line_theta)) {
    if (EMIT) off = (u32)__builtin_amdgcn_readfirstlane((int)p.items[item]);
    const u32 cap = EMIT ? (u32)min(p.seg_capacity, (size_t)0xFFFFFFFFu) : 0xFFFFFFFFu;
    int4 *out = reinterpret_cast<int4 *>(p.segs) + (size_t)frame * p.seg_capacity;
    SegWalk w;
    w.fbase = p.map + (size_t)frame * p.frame_stride;
    w.pitch = (u32)p.pitch;
    w.major = p.tab_major[n];
    w.L = w.major ? p.H : p.W;
    w.M = w.major ? p.W : p.H;
    w.slope = p.tab_slope[n];
    w.c0 = __fmul_rn(line_rho, p.tab_scale[n]);
    const u64 below = ((u64)1 << lane) - 1;
    int prev_t = -1, start_t = -1;  // last edge step and first step of the open group; -1: no edge yet
    // one chunk of 64 steps from t0 on: e is the lane's edge flag
    auto chunk = [&](int t0, bool e) {
      const u64 E = __ballot(e);
      if (E == 0) return;
      const int t = t0 + lane;
      const u64 eb = E & below;
      const int prev = eb ? t0 + 63 - __clzll((long long)eb) : prev_t;
      const bool starts = e && (prev < 0 || t - prev - 1 > p.max_gap);
      const u64 S = __ballot(starts);
      const u64 sb = S & below;
      int4 seg = make_int4(0, 0, 0, 0);
      const bool keep = starts && prev >= 0 && w.close(sb ? t0 + 63 - __clzll((long long)sb) : start_t, prev, p.min_length, seg);
      const u64 K = __ballot(keep);
      if (EMIT && keep) {
        const u32 slot = off + mbcnt64(K);
        if (slot < cap) out[slot] = seg;
      }
      off += (u32)__popcll(K);
      prev_t = t0 + 63 - __clzll((long long)E);
      if (S) start_t = t0 + 63 - __clzll((long long)S);
    };
    for (int t0 = 0; t0 < w.L && off < cap; t0 += 256) {  // four chunks in flight
      bool e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = w.edge(t0 + 64 * j + lane);
      if (__ballot(e[0] || e[1] || e[2] || e[3]) == 0) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) chunk(t0 + 64 * j, e[j]);
    }
    if (prev_t >= 0) {  // the group still open: wave-uniform
      int4 seg = make_int4(0, 0, 0, 0);
      if (w.close(start_t, prev_t, p.min_length, seg)) {
        if (EMIT && lane == 0 && off < cap) out[off] = seg;
        ++off;
      }
    }
  }
  if (!EMIT && lane == 0) p.items[item] = off;
}

__global__ __launch_bounds__(256) void k_seg_count(const SegParams p) { seg_walk<false>(p); }
__global__ __launch_bounds__(256) void k_seg_emit(const SegParams p) { seg_walk<true>(p); }

__global__ __launch_bounds__(256) void k_seg_scan(const SegParams p)
{
  const int lane = threadIdx.x & 63;
  const int frame = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (frame >= p.nframes) return;
  u32 *it = p.items + (size_t)frame * p.line_capacity;
  const size_t nl = min((size_t)p.line_counts[frame], p.line_capacity);
  u32 carry = 0;  // (a frame has fewer than 2^32 segments: plan_hough_segments)
  for (size_t c0 = 0; c0 < nl; c0 += 64) {
    const size_t c = c0 + lane;
    const u32 v = c < nl ? it[c] : 0u;
    u32 incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (c < nl) it[c] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
  if (lane == 0) p.seg_counts[frame] = carry;
}

}  // namespace

// The three launches on stream s.  seg_capacity == 0: counts only (k_seg_emit is not launched, p.segs is not looked at).
hipError_t launch_hough_segments(const SegParams &p, hipStream_t s)
{
  if (!p.map || !p.lines || !p.line_counts || !p.tab_theta || !p.tab_major || !p.tab_slope || !p.tab_scale || !p.items || !p.seg_counts
      || (((uintptr_t)p.lines | (uintptr_t)p.line_counts | (uintptr_t)p.items | (uintptr_t)p.seg_counts) & 3u) || p.W < 1 || p.H < 1 || p.nframes < 1 || p.numangle < 1
      || p.pitch < (size_t)p.W || (unsigned long long)p.H * p.pitch >= (1ull << 32) || p.min_length < 0 || p.max_gap < 0 || p.line_capacity < 1 || p.total_items < 1
      || p.total_items > 0x7FFFFFF0 || (unsigned long long)p.total_items != (unsigned long long)p.nframes * p.line_capacity || (p.seg_capacity && (!p.segs || ((uintptr_t)p.segs & 15u))))
    return hipErrorInvalidValue;
  const dim3 lines_grid((unsigned)(((long long)p.total_items + 3) / 4)), block(256);
  hipLaunchKernelGGL(k_seg_count, lines_grid, block, 0, s, p);
  hipLaunchKernelGGL(k_seg_scan, dim3((p.nframes + 3) / 4), block, 0, s, p);
  if (p.seg_capacity) hipLaunchKernelGGL(k_seg_emit, lines_grid, block, 0, s, p);
  return hipGetLastError();
}

}  // namespace hc
