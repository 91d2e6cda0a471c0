// dist.hip -- the exact Euclidean distance transform of u8 maps: per pixel the squared distance to the nearest feature pixel (or
// its root), and that pixel (hc_distance_transform_device: cv::distanceTransform(DIST_L2, DIST_MASK_PRECISE) with
// DIST_LABEL_PIXEL labels on the device).
//
// The only per-pixel storage is the caller's distance plane; there is no scratch, no atomic and no pass structure.
//
//   k_dt_cols   a lane owns a column.  It walks down, carrying the row of the last feature pixel it met, and writes dy = y' - y
//               (<= 0) of that pixel, or DT_NO_DY, into the plane.  Then it walks up, carrying the row of the nearest feature
//               pixel below, and overwrites the words where below is STRICTLY nearer than above: a tie stays with the one above.
//               A feature pixel is the word 0 on the way up, so the map is read once.  Map bytes (down) and plane words (up) do
//               not depend on the carried row: DT_LOOKAHEAD rows are loaded before they are walked.  Lanes are adjacent columns, so
//               every load and store of a wave is one run of bytes or words.
//   k_dt_rows   a workgroup owns DT_ROWS whole rows, one after the other.  It loads the row's dy into LDS, and only behind the barrier
//               overwrites the row with the result.  The lane of pixel x looks at x' = x - d and x + d for d = 1, 2, ... and takes
//               d^2 + dy(x')^2; it stops when d^2 exceeds the best value so far or both sides have left the row.  Adjacent lanes
//               read adjacent words of LDS on both sides: no bank conflicts.
//
// The tie rule (the smallest x', then the smallest y') follows from the order of the search.  Column x' offers exactly one pixel,
// its nearest with the smaller y' on a tie.  On the left, x - d is smaller than every x' looked at before, so it replaces the
// best on <=; on the right, x + d is larger than all of them, so it replaces on < only.  The loop runs while d^2 <= best for
// that reason: a feature pixel at exactly distance d on the left ties, and wins.
// A row in which no word holds a dy is a row of a frame without a feature pixel (a column with one has a dy in every row): every
// wave decides that once per row, by ballot, and writes HC_DT_NONE / +inf / -1 without a search.
// DT_NO_DY is never squared and never compared as a distance: a word that holds it is skipped.  Everything else fits int32:
// d <= W - 1, |dy| <= H - 1 and (W - 1)^2 + (H - 1)^2 < 2^31 - 1 (plan_distance_transform).
#include "canny_device.h"

namespace hc {

namespace {

static __device__ __forceinline__ int32_t *plane(int32_t *base, size_t frame_stride, int frame)
{
  return reinterpret_cast<int32_t *>(reinterpret_cast<char *>(base) + (size_t)frame * frame_stride);
}

__global__ __launch_bounds__(DT_COL_THREADS) void k_dt_cols(const DistParams p)
{
  const int x = (int)(blockIdx.x * DT_COL_THREADS + threadIdx.x);
  if (x >= p.W) return;
  const int frame = blockIdx.y;
  const uint8_t *m = p.map + (size_t)frame * p.frame_stride + x;
  int32_t *out = plane(p.dist, p.dist_frame_stride, frame) + x;
  const size_t pitch4 = p.dist_pitch >> 2;
  const bool to_zero = p.target == DT_TO_ZERO;
  int last = -1;  // the row of the nearest feature pixel above, this row included; -1: none yet
  for (int y0 = 0; y0 < p.H; y0 += DT_LOOKAHEAD) {
    uint8_t b[DT_LOOKAHEAD];
#pragma unroll
    for (int k = 0; k < DT_LOOKAHEAD; ++k) b[k] = y0 + k < p.H ? m[(size_t)(y0 + k) * p.pitch] : (uint8_t)0;
#pragma unroll
    for (int k = 0; k < DT_LOOKAHEAD; ++k) {
      const int y = y0 + k;
      if (y >= p.H) break;
      if ((b[k] != 0) != to_zero) last = y;
      out[(size_t)y * pitch4] = last >= 0 ? last - y : DT_NO_DY;
    }
  }
  int next = -1;  // the row of the nearest feature pixel below, this row included
  for (int y1 = p.H - 1; y1 >= 0; y1 -= DT_LOOKAHEAD) {
    int v[DT_LOOKAHEAD];
#pragma unroll
    for (int k = 0; k < DT_LOOKAHEAD; ++k) v[k] = y1 - k >= 0 ? out[(size_t)(y1 - k) * pitch4] : 0;
#pragma unroll
    for (int k = 0; k < DT_LOOKAHEAD; ++k) {
      const int y = y1 - k;
      if (y < 0) break;
      if (v[k] == 0) next = y;
      else if (next >= 0 && (v[k] == DT_NO_DY || next - y < -v[k])) out[(size_t)y * pitch4] = next - y;
    }
  }
}

__global__ __launch_bounds__(DT_ROW_THREADS) void k_dt_rows(const DistParams p)
{
  extern __shared__ int dyrow[];  // [W]
  const int frame = blockIdx.y, t = threadIdx.x;
  int32_t *fd = plane(p.dist, p.dist_frame_stride, frame);
  int32_t *fn = p.nearest ? plane(p.nearest, p.nearest_frame_stride, frame) : nullptr;
  const size_t dpitch4 = p.dist_pitch >> 2, npitch4 = p.nearest_pitch >> 2;
  const bool root = p.dist_type == DT_F32;
  for (int r = 0; r < DT_ROWS; ++r) {
    const int y = (int)blockIdx.x * DT_ROWS + r;
    if (y >= p.H) break;  // (the whole workgroup)
    int32_t *drow = fd + (size_t)y * dpitch4;
    bool has = false;
    for (int x = t; x < p.W; x += DT_ROW_THREADS) {
      const int v = drow[x];
      dyrow[x] = v;
      has = has || v != DT_NO_DY;
    }
    __syncthreads();
    // Does the row hold a dy at all?  Once per wave and row: the words the wave loaded itself answer in a frame with features
    // in most columns; otherwise the wave reads the LDS row 64 words at a time until it meets one.  (No flag in LDS: the row may
    // take all 64 KiB.)
    bool any = __ballot(has) != 0;
    for (int x0 = 0; x0 < p.W && !any; x0 += 64) any = __ballot(x0 + (t & 63) < p.W && dyrow[x0 + (t & 63)] != DT_NO_DY) != 0;
    for (int x = t; x < p.W; x += DT_ROW_THREADS) {
      int best = DT_NONE, bx = x;
      if (any) {
        const int dy0 = dyrow[x];
        if (dy0 != DT_NO_DY) best = dy0 * dy0;
        for (int d = 1; d * d <= best && (d <= x || x + d < p.W); ++d) {
          if (d <= x) {
            const int dl = dyrow[x - d];
            if (dl != DT_NO_DY) {
              const int c = d * d + dl * dl;
              if (c <= best) { best = c; bx = x - d; }
            }
          }
          if (x + d < p.W) {
            const int dr = dyrow[x + d];
            if (dr != DT_NO_DY) {
              const int c = d * d + dr * dr;
              if (c < best) { best = c; bx = x + d; }
            }
          }
        }
      }
      // (best == DT_NONE iff !any; (float)DT_NONE is 2^31, whose root is finite: the infinity is written as such)
      drow[x] = !root ? best : best == DT_NONE ? 0x7F800000 : __float_as_int(sqrtf((float)best));
      if (fn) fn[(size_t)y * npitch4 + x] = any ? (y + dyrow[bx]) * p.W + bx : -1;
    }
    __syncthreads();  // the next row's dy go where this row's were read
  }
}

}  // namespace

// The two kernels on stream s.  Everything the kernels rely on for their bounds is checked again here.
hipError_t launch_distance_transform(const DistParams &p, hipStream_t s)
{
  const long long w1 = (long long)p.W - 1, h1 = (long long)p.H - 1;
  if (!p.map || !p.dist || (((uintptr_t)p.dist | p.dist_pitch | p.dist_frame_stride | (uintptr_t)p.nearest | p.nearest_pitch | p.nearest_frame_stride) & 3u)
      || p.W < 1 || p.H < 1 || p.W > DT_MAX_W || p.nframes < 1 || p.nframes > 65535 || p.pitch < (size_t)p.W || p.dist_pitch < 4 * (size_t)p.W
      || (p.nearest && p.nearest_pitch < 4 * (size_t)p.W) || w1 * w1 + h1 * h1 >= 0x7FFFFFFFll || (long long)p.W * p.H >= 0x7FFFFFFFll
      || (unsigned long long)p.H * p.pitch >= (1ull << 32) || (unsigned long long)p.H * p.dist_pitch >= (1ull << 32)
      || (p.nearest && (unsigned long long)p.H * p.nearest_pitch >= (1ull << 32))
      || (p.target != DT_TO_NONZERO && p.target != DT_TO_ZERO) || (p.dist_type != DT_SQUARED_I32 && p.dist_type != DT_F32)
      || p.col_groups != (unsigned)((p.W + DT_COL_THREADS * DT_COLS_PER_LANE - 1) / (DT_COL_THREADS * DT_COLS_PER_LANE))
      || p.row_groups != (unsigned)((p.H + DT_ROWS - 1) / DT_ROWS) || p.lds_bytes != 4u * (unsigned)p.W)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dt_cols, dim3(p.col_groups, p.nframes), dim3(DT_COL_THREADS), 0, s, p);
  hipLaunchKernelGGL(k_dt_rows, dim3(p.row_groups, p.nframes), dim3(DT_ROW_THREADS), p.lds_bytes, s, p);
  return hipGetLastError();
}

}  // namespace hc
