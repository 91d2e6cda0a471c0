// stats.hip -- frame statistics for the automatic thresholds of Mode O.
//
//   k_hist256   256-bin histograms of u8 frames (hc_histogram_device): d_hist[f][v] = samples of value v in frame f, the
//               channels of 3-channel frames pooled.
//   k_auto_thr  one wave per frame: prefix sums of the 256 bins, then the median or the Otsu rule of auto_thr.h -> the
//               frame's (low, high) in the table hc_frame_thresholds_device installs.
//
// k_hist256: a work item is (frame, chunk of rows) and belongs to one wave.  Per row the wave reads the dwords that lie whole
// inside [row, row + row_bytes) -- lane l the dwords l, l + 64, ... of the aligned body, four in flight -- and the up to three
// bytes before and after them bytewise (lanes 0..2 and 32..34), so no byte outside the row is read at any alignment of base,
// pitch and frame stride.  Every sample is one LDS atomic add into the wave's private histogram.  Neighbouring pixels
// are alike, so the lanes of one instruction often meet in a bin, and same-address adds are served one after the other: the
// histogram is kept HIST_SUBS = 8 times, lane l counts into copy l % 8, bin-major (copy c of bin v at dword 8 v + c), so a
// flat frame -- all 64 lanes on one bin -- is 8 addresses in 8 banks with 8 lanes each instead of 64 on one.  8 KiB per wave,
// 32 KiB per 4-wave workgroup: five workgroups per CU (160 KiB LDS), 20 waves.  At the end of the item lane l sums the copies
// of bins l, l + 64, l + 128, l + 192 and adds the non-zero sums to d_hist[frame] with vector global atomics (256
// contiguous bytes per wave-instruction).  Counts are integer sums: the result does not depend on the split.
// Measured (profiles/auto_thr/README.md): 1024 frames of 1920 x 1080 in 0.96 ms on natural and noise frames, 1.06 ms on flat
// ones -- the same-bin worst case costs 10 % with 8 copies; fewer copies, and more, have not been tried.
#include "canny_device.h"
#include "auto_thr.h"

namespace hc {

namespace {

constexpr int HIST_SUBS = 8;

__global__ __launch_bounds__(256) void k_hist256(const HistParams p)
{
  __shared__ u32 lds[4][256 * HIST_SUBS];
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const int item = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + wib);
  if (item >= p.total_items) return;
  const int chunk = item % p.nchunks;
  const int frame = item / p.nchunks;
  const int r0 = chunk * p.chunk_rows, rend = min(r0 + p.chunk_rows, p.H);
  u32 *h = lds[wib];
#pragma unroll
  for (int i = 0; i < 256 * HIST_SUBS / 64; ++i) h[i * 64 + lane] = 0u;
  wave_lds_sync();

  u32 *mine = h + (lane & (HIST_SUBS - 1));
  auto count_byte = [&](u32 v) { (void)__hip_atomic_fetch_add(mine + v * HIST_SUBS, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
  auto count_dword = [&](u32 d) {
    count_byte(d & 0xFFu);
    count_byte((d >> 8) & 0xFFu);
    count_byte((d >> 16) & 0xFFu);
    count_byte(d >> 24);
  };
  const uint8_t *fbase = p.in + (size_t)frame * p.in_frame_stride;
  const int nb = p.row_bytes;
  for (int row = r0; row < rend; ++row) {  // everything but `lane` is wave-uniform
    const uint8_t *rp = fbase + (size_t)row * p.in_pitch;
    const int head = min((int)((0u - (u32)(uintptr_t)rp) & 3u), nb);  // bytes before the first aligned dword
    const int nd = (nb - head) >> 2;                                   // whole dwords inside the row
    const int tail = nb - head - 4 * nd;                               // bytes after the last of them
    if (lane < head) count_byte(rp[lane]);
    if (lane >= 32 && lane - 32 < tail) count_byte(rp[head + 4 * nd + (lane - 32)]);
    const u32 *body = reinterpret_cast<const u32 *>(rp + head);
    int i = lane;
    for (; i + 192 < nd; i += 256) {
      const u32 d0 = body[i], d1 = body[i + 64], d2 = body[i + 128], d3 = body[i + 192];
      count_dword(d0); count_dword(d1); count_dword(d2); count_dword(d3);
    }
    for (; i < nd; i += 64) count_dword(body[i]);
  }
  wave_lds_sync();

  u32 *out = p.hist + (size_t)frame * 256;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int bin = lane + 64 * k;
    u32 sum = 0;
#pragma unroll
    for (int c = 0; c < HIST_SUBS; ++c) sum += h[bin * HIST_SUBS + c];
    if (sum) (void)__hip_atomic_fetch_add(out + bin, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One wave per frame, lane l the bins 4 l .. 4 l + 3: the bins' running sums inside the lane, a wave scan across the lanes,
// then every lane tests its own bins (median) or scores its own thresholds (Otsu) with the functions of auto_thr.h and the
// wave keeps the one answer.
__global__ __launch_bounds__(256) void k_auto_thr(const u32 *hist, int nframes, int rule, double param, int32_t *thr)
{
  const int lane = threadIdx.x & 63;
  const int frame = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (frame >= nframes) return;
  const u32 *h = hist + (size_t)frame * 256;
  long long c[4], s[4];  // counts / value sums of the lane's bins up to and including bin 4 l + k
  long long cw = 0, sw = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int bin = 4 * lane + k;
    const long long hv = h[bin];
    cw += hv; sw += bin * hv;
    c[k] = cw; s[k] = sw;
  }
  long long ci = cw, si = sw;  // inclusive scan over the lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long tc = __shfl_up(ci, off), ts = __shfl_up(si, off);
    if (lane >= off) { ci += tc; si += ts; }
  }
  const long long cex = ci - cw, sex = si - sw;  // sums of the lanes below
  const long long N = __shfl(ci, 63), S = __shfl(si, 63);
  int low = 0, high = 0;
  if (rule == AUTO_MEDIAN) {
    int a = 256, b = 256;  // exactly one bin of the frame holds each of the two samples (N >= 1)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long below = cex + (k ? c[k - 1] : 0), upto = cex + c[k];
      if (auto_bin_holds(below, upto, (N - 1) / 2)) a = 4 * lane + k;
      if (auto_bin_holds(below, upto, N / 2)) b = 4 * lane + k;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      a = min(a, __shfl_xor(a, off));
      b = min(b, __shfl_xor(b, off));
    }
    auto_median_pair(a, b, param, &low, &high);
  } else {
    double best = 0.0;
    int best_t = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int t = 4 * lane + k;
      const long long w0 = cex + c[k], s0 = sex + s[k];
      if (t < 255 && w0 > 0 && N - w0 > 0) {
        const double score = auto_otsu_score(N, S, w0, s0);
        if (auto_otsu_takes(score, t, best, best_t)) { best = score; best_t = t; }
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {  // (score descending, t ascending) is a total order: every lane ends with the same pair
      const double ob = __shfl_xor(best, off);
      const int ot = __shfl_xor(best_t, off);
      if (ot >= 0 && auto_otsu_takes(ob, ot, best, best_t)) { best = ob; best_t = ot; }
    }
    auto_otsu_pair(best_t, param, &low, &high);
  }
  if (lane == 0) { thr[2 * (size_t)frame] = low; thr[2 * (size_t)frame + 1] = high; }
}

}  // namespace

hipError_t launch_hist256(const HistParams &p, hipStream_t s)
{
  if (!p.in || !p.hist || ((uintptr_t)p.hist & 3u) || p.row_bytes < 1 || p.H < 1 || p.nframes < 1 || p.in_pitch < (size_t)p.row_bytes
      || (unsigned long long)p.H * p.in_pitch >= (1ull << 32) || p.chunk_rows < 1 || p.nchunks != (p.H + p.chunk_rows - 1) / p.chunk_rows
      || (long long)p.total_items != (long long)p.nframes * p.nchunks)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_hist256, dim3((p.total_items + 3) / 4), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_auto_thr(const u32 *hist, int nframes, int rule, double param, int32_t *thr, hipStream_t s)
{
  if (!hist || !thr || (((uintptr_t)hist | (uintptr_t)thr) & 3u) || nframes < 1 || !auto_param_ok(rule, param)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_auto_thr, dim3((nframes + 3) / 4), dim3(256), 0, s, hist, nframes, rule, param, thr);
  return hipGetLastError();
}

}  // namespace hc
