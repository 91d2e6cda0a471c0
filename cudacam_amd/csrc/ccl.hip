// ccl.hip -- the connected components of u8 maps: a number per pixel, the number of components, and per component the bounding
// box, the area and the centroid (hc_connected_components_device: cv::connectedComponentsWithStats on the device).
//
// The only per-pixel storage is the caller's label plane.  Until k_ccl_roots, a foreground pixel's word holds a LINK: 1 + the
// word index (y * label_pitch / 4 + x, CclParams) of a pixel of its component that does not come after it in raster order;
// background holds 0.  A pixel whose link names itself is a ROOT.  Links only ever decrease, so a walk along them ends.
//
//   k_ccl_local    a workgroup owns a tile of 64 x 32 pixels.  A wave reads a row of the tile, one byte per lane; the ballot of
//                  the non-zero bytes gives the row's runs, and every pixel starts as a link to the first pixel of its run.
//                  Runs that touch a run of the row above are united in LDS (atomicMin union-find); then every pixel writes the
//                  link to its tile-local root, or 0, to the plane.
//   k_ccl_merge    a thread per pixel that lies just below a horizontal or just right of a vertical tile border: the same
//                  unions, across the border, with atomicMin on the plane.  The corner where four tiles meet needs no case of
//                  its own: the pixel below a horizontal border looks at its three upper neighbours whatever tile they are in.
//   k_ccl_flatten  a wave per chunk of rows: every foreground pixel walks to its root and links to it directly; the roots of
//                  the chunk are counted -> items[frame][chunk].
//   k_ccl_scan     one wave per frame: exclusive prefix sum of the frame's items in place; counts[frame] = roots + 1.
//   k_ccl_roots    the work split of k_ccl_flatten again: the roots of a chunk, in raster order, take the numbers offset + 1,
//                  offset + 2, ... and store them NEGATED, which tells a numbered root from a link.
//   k_ccl_number   every other foreground pixel reads its root's number and stores it; a root turns its own positive.  A reader
//                  takes the absolute value, so it does not matter which of the two it meets.
//   k_ccl_rows     the rows 0 .. min(N, capacity) - 1 of the frame's statistics become (INT_MAX, INT_MAX, -1, -1, 0), its
//                  centroid rows two zero int64 sums.
//   k_ccl_stats    a wave per chunk of rows: 64 pixels of a row per trip, cut into runs of equal numbers; the first lane of a run
//                  adds the run -- left, right, row, length, sum of x, sum of y -- to its component's rows with one set of integer
//                  atomics.  Background runs go to registers instead and reach row 0 once per wave, at the end of its chunk.
//   k_ccl_finish   (min x, min y, max x, max y, area) -> (left, top, width, height, area), the two sums -> two float64 divisions.
//
// Why the result is a function of the map alone although the merges race: a link always names a pixel of the same component
// that comes earlier, atomicMin can only lower it, and a union returns only once both pixels have one root.  So when k_ccl_merge
// ends every component has exactly one root, and it is its smallest pixel in raster order, whatever the order of the merges.
// The numbers follow from the roots' positions alone; the statistics are integer sums, minima and maxima, which do not depend
// on arrival order.
// No kernel waits for another workgroup: every loop ends on its own data (a find walks strictly descending links; a union
// either links, or goes on with a strictly smaller pixel).  Values that are no link below the pixel they stand on -- a plane of
// garbage -- end a walk where they are met.
#include "canny_device.h"

namespace hc {

namespace {

// ---- union-find on a tile's labels in LDS: L[i] <= i, a root names itself ----
static __device__ __forceinline__ int lds_find(const int *L, int x)
{
  int v;
  while ((v = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < x) x = v;
  return x;
}
static __device__ __forceinline__ void lds_union(int *L, int a, int b)
{
  for (;;) {
    a = lds_find(L, a);
    b = lds_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;  // a was still a root: linked
    a = old;               // someone linked a below meanwhile (old < a): that pixel and b remain to be united
  }
}

// ---- union-find on the plane: L[i] - 1 is the link of word i ----
static __device__ __forceinline__ int g_load(const int32_t *L, int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// A stale value is an earlier link of the same word: still a pixel of the component, still below.
static __device__ __forceinline__ int g_find(const int32_t *L, int x)
{
  for (;;) {
    const int v = g_load(L, x) - 1;
    if (v < 0 || v >= x) return x;  // a root (v == x); anything else that is no link below x ends the walk as well
    x = v;
  }
}
static __device__ __forceinline__ void g_union(int32_t *L, int a, int b)
{
  for (;;) {
    a = g_find(L, a);
    b = g_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b + 1) - 1;
    if (old < 0 || old >= a) return;  // a was still a root (old == a): linked
    a = old;                          // linked below meanwhile (old < a): a + b has decreased, so the loop ends
  }
}

static __device__ __forceinline__ int32_t *frame_labels(const CclParams &p, int frame)
{
  return reinterpret_cast<int32_t *>(reinterpret_cast<char *>(p.labels) + (size_t)frame * p.label_frame_stride);
}

__global__ __launch_bounds__(CCL_THREADS) void k_ccl_local(const CclParams p)
{
  __shared__ int L[CCL_TILE_H * CCL_TILE_W];
  __shared__ u64 M[CCL_TILE_H];  // the foreground of the tile's rows, bit per column
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x, frame = blockIdx.y;
  const int tx0 = (tile % p.tiles_x) * CCL_TILE_W, ty0 = (tile / p.tiles_x) * CCL_TILE_H;
  const uint8_t *fmap = p.map + (size_t)frame * p.frame_stride;
  const int x = tx0 + lane;
  for (int r = wave; r < CCL_TILE_H; r += CCL_THREADS / 64) {
    const int y = ty0 + r;
    const bool fg = y < p.H && x < p.W && fmap[(size_t)y * p.pitch + x] != 0;
    const u64 m = __ballot(fg);
    if (lane == 0) M[r] = m;
    const u64 gaps = ~m & ((1ull << lane) - 1);  // the background pixels left of this one: its run starts behind the last of them
    const int start = gaps ? 64 - __clzll((long long)gaps) : 0;
    L[r * CCL_TILE_W + lane] = r * CCL_TILE_W + (fg ? start : lane);
  }
  __syncthreads();
  const bool eight = p.connectivity == 8;
  for (int r = wave; r < CCL_TILE_H; r += CCL_THREADS / 64) {
    if (r == 0) continue;
    const u64 m = M[r], up = M[r - 1];
    if (!((m >> lane) & 1)) continue;
    // One union per pair of touching runs is enough: a pixel leaves it to its left neighbour where that one sees the same run above
    const bool left = lane > 0 && ((m >> (lane - 1)) & 1), right = lane < 63 && ((m >> (lane + 1)) & 1);
    const bool u = (up >> lane) & 1, ul = lane > 0 && ((up >> (lane - 1)) & 1), ur = lane < 63 && ((up >> (lane + 1)) & 1);
    const int me = r * CCL_TILE_W + lane, above = me - CCL_TILE_W;
    if (u) {
      if (!(left && ul)) lds_union(L, me, above);
    } else if (eight) {
      if (ul && !left) lds_union(L, me, above - 1);
      if (ur && !right) lds_union(L, me, above + 1);
    }
  }
  __syncthreads();
  int32_t *fl = frame_labels(p, frame);
  const int pitch4 = (int)(p.label_pitch >> 2);
  for (int r = wave; r < CCL_TILE_H; r += CCL_THREADS / 64) {
    const int y = ty0 + r;
    if (y >= p.H || x >= p.W) continue;
    int v = 0;
    if ((M[r] >> lane) & 1) {
      const int root = lds_find(L, r * CCL_TILE_W + lane);
      v = 1 + (ty0 + root / CCL_TILE_W) * pitch4 + tx0 + root % CCL_TILE_W;
    }
    fl[(size_t)y * pitch4 + x] = v;
  }
}

__global__ __launch_bounds__(CCL_THREADS) void k_ccl_merge(const CclParams p)
{
  const unsigned i = blockIdx.x * CCL_THREADS + threadIdx.x;
  if (i >= p.border_items) return;
  int32_t *L = frame_labels(p, blockIdx.y);
  const int pitch4 = (int)(p.label_pitch >> 2);
  const unsigned below = (unsigned)(p.tiles_y - 1) * (unsigned)p.W;  // the items below a horizontal border come first
  const bool eight = p.connectivity == 8;
  if (i < below) {  // the rule of k_ccl_local, on the plane (a word is foreground iff it is not 0, which no kernel changes)
    const int y = (int)(i / (unsigned)p.W + 1) * CCL_TILE_H, x = (int)(i % (unsigned)p.W);
    const int me = y * pitch4 + x, above = me - pitch4;
    if (L[me] == 0) return;
    const bool left = x > 0 && L[me - 1] != 0, right = x + 1 < p.W && L[me + 1] != 0;
    const bool u = L[above] != 0, ul = x > 0 && L[above - 1] != 0, ur = x + 1 < p.W && L[above + 1] != 0;
    if (u) {
      if (!(left && ul)) g_union(L, me, above);
    } else if (eight) {
      if (ul && !left) g_union(L, me, above - 1);
      if (ur && !right) g_union(L, me, above + 1);
    }
  } else {  // right of a vertical border: the left neighbour, or (it is joined to both) the two diagonal ones
    const unsigned j = i - below;
    const int x = (int)(j / (unsigned)p.H + 1) * CCL_TILE_W, y = (int)(j % (unsigned)p.H);
    const int me = y * pitch4 + x;
    if (L[me] == 0) return;
    if (L[me - 1] != 0) g_union(L, me, me - 1);
    else if (eight) {
      if (y > 0 && L[me - 1 - pitch4] != 0) g_union(L, me, me - 1 - pitch4);
      if (y + 1 < p.H && L[me - 1 + pitch4] != 0) g_union(L, me, me - 1 + pitch4);
    }
  }
}

// What the four kernels that walk the plane in chunks of rows share: the wave's item, its rows and its frame
struct Chunk { int item, frame, r0, rend; };
static __device__ __forceinline__ Chunk wave_chunk(const CclParams &p)
{
  Chunk c;
  c.item = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (int)(threadIdx.x >> 6));
  c.frame = c.item / p.nchunks;
  c.r0 = (c.item % p.nchunks) * p.chunk_rows;
  c.rend = min(c.r0 + p.chunk_rows, p.H);
  return c;
}

__global__ __launch_bounds__(CCL_THREADS) void k_ccl_flatten(const CclParams p)
{
  const int lane = threadIdx.x & 63;
  const Chunk c = wave_chunk(p);
  if (c.item >= p.total_items) return;
  int32_t *L = frame_labels(p, c.frame);
  const int pitch4 = (int)(p.label_pitch >> 2);
  u32 n = 0;
  for (int row = c.r0; row < c.rend; ++row)
    for (int x0 = 0; x0 < p.W; x0 += 64) {
      const int x = x0 + lane, i = row * pitch4 + x;
      bool root = false;
      if (x < p.W && L[i] != 0) {
        const int r = g_find(L, i);
        root = r == i;
        if (!root) __hip_atomic_store(L + i, r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (a walk that passes here meets the old link or this one)
      }
      n += (u32)__popcll(__ballot(root));
    }
  if (lane == 0) p.items[c.item] = n;
}

__global__ __launch_bounds__(CCL_THREADS) void k_ccl_scan(const CclParams p)  // k_edge_scan's loop (edge_points.hip)
{
  const int lane = threadIdx.x & 63;
  const int frame = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (frame >= p.nframes) return;
  u32 *it = p.items + (size_t)frame * p.nchunks;
  u32 carry = 0;
  for (int c0 = 0; c0 < p.nchunks; c0 += 64) {
    const int c = c0 + lane;
    const u32 v = c < p.nchunks ? it[c] : 0u;
    u32 incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (c < p.nchunks) it[c] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
  if (lane == 0) p.counts[frame] = carry + 1;  // the background counts, as in cv::connectedComponents' return value
}

__global__ __launch_bounds__(CCL_THREADS) void k_ccl_roots(const CclParams p)
{
  const int lane = threadIdx.x & 63;
  const Chunk c = wave_chunk(p);
  if (c.item >= p.total_items) return;
  int32_t *L = frame_labels(p, c.frame);
  const int pitch4 = (int)(p.label_pitch >> 2);
  u32 off = (u32)__builtin_amdgcn_readfirstlane((int)p.items[c.item]);  // the roots of the frame before this chunk: wave-uniform
  for (int row = c.r0; row < c.rend; ++row)
    for (int x0 = 0; x0 < p.W; x0 += 64) {
      const int x = x0 + lane, i = row * pitch4 + x;
      const bool root = x < p.W && L[i] == i + 1;
      const u64 m = __ballot(root);
      if (root) L[i] = -(int)(off + mbcnt64(m) + 1);
      off += (u32)__popcll(m);
    }
}

__global__ __launch_bounds__(CCL_THREADS) void k_ccl_number(const CclParams p)
{
  const int lane = threadIdx.x & 63;
  const Chunk c = wave_chunk(p);
  if (c.item >= p.total_items) return;
  int32_t *L = frame_labels(p, c.frame);
  const int pitch4 = (int)(p.label_pitch >> 2);
  for (int row = c.r0; row < c.rend; ++row)
    for (int x0 = 0; x0 < p.W; x0 += 64) {
      const int x = x0 + lane, i = row * pitch4 + x;
      if (x >= p.W) continue;
      const int v = L[i];  // only this thread writes word i: a link to the root (> 0), the root's negated number (< 0) or 0
      if (v > 0) {
        const int n = g_load(L, v - 1);  // the root's number, negated or already positive
        L[i] = n < 0 ? -n : n;
      } else if (v < 0)
        __hip_atomic_store(L + i, -v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(CCL_THREADS) void k_ccl_rows(const CclParams p)
{
  const int frame = blockIdx.y;
  const size_t rows = min((size_t)p.counts[frame], p.capacity);
  int32_t *st = p.stats + (size_t)frame * p.capacity * 5;
  unsigned long long *sm = p.sums + (size_t)frame * p.capacity * 2;
  for (size_t k = (size_t)blockIdx.x * CCL_THREADS + threadIdx.x; k < rows; k += (size_t)gridDim.x * CCL_THREADS) {
    int32_t *s = st + 5 * k;
    s[0] = 0x7FFFFFFF; s[1] = 0x7FFFFFFF; s[2] = -1; s[3] = -1; s[4] = 0;
    sm[2 * k] = 0; sm[2 * k + 1] = 0;
  }
}

static __device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int off)
{
  const u32 lo = __shfl_xor((u32)v, off), hi = __shfl_xor((u32)(v >> 32), off);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(CCL_THREADS) void k_ccl_stats(const CclParams p)
{
  const int lane = threadIdx.x & 63;
  const Chunk c = wave_chunk(p);
  if (c.item >= p.total_items) return;
  const int32_t *L = frame_labels(p, c.frame);
  const int pitch4 = (int)(p.label_pitch >> 2);
  int32_t *st = p.stats + (size_t)c.frame * p.capacity * 5;
  unsigned long long *sm = p.sums + (size_t)c.frame * p.capacity * 2;
  // the background of this wave's rows
  int b_minx = 0x7FFFFFFF, b_miny = 0x7FFFFFFF, b_maxx = -1, b_maxy = -1;
  unsigned long long b_area = 0, b_sx = 0, b_sy = 0;
  for (int row = c.r0; row < c.rend; ++row)
    for (int x0 = 0; x0 < p.W; x0 += 64) {
      const int x = x0 + lane;
      const int valid = min(64, p.W - x0);
      const int lab = x < p.W ? L[row * pitch4 + x] : -1;
      const int prev = __shfl_up(lab, 1);
      const bool head = x < p.W && (lane == 0 || lab != prev);
      const u64 heads = __ballot(head);
      if (!head) continue;
      const u64 later = (heads >> lane) >> 1;  // the heads right of this lane
      const int len = (later ? lane + 1 + __builtin_ctzll(later) : valid) - lane;
      const int xe = x + len - 1;
      const unsigned long long sx = (unsigned long long)len * (unsigned long long)(x + xe) / 2, sy = (unsigned long long)len * (unsigned long long)row;
      if (lab == 0) {
        b_minx = min(b_minx, x); b_maxx = max(b_maxx, xe); b_miny = min(b_miny, row); b_maxy = max(b_maxy, row);
        b_area += (unsigned long long)len; b_sx += sx; b_sy += sy;
      } else if ((size_t)(u32)lab < p.capacity) {
        int32_t *s = st + 5 * (size_t)lab;
        atomicMin(&s[0], x); atomicMin(&s[1], row); atomicMax(&s[2], xe); atomicMax(&s[3], row); atomicAdd(&s[4], len);
        atomicAdd(&sm[2 * (size_t)lab], sx); atomicAdd(&sm[2 * (size_t)lab + 1], sy);
      }
    }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    b_minx = min(b_minx, __shfl_xor(b_minx, off)); b_miny = min(b_miny, __shfl_xor(b_miny, off));
    b_maxx = max(b_maxx, __shfl_xor(b_maxx, off)); b_maxy = max(b_maxy, __shfl_xor(b_maxy, off));
    b_area += shfl_xor64(b_area, off); b_sx += shfl_xor64(b_sx, off); b_sy += shfl_xor64(b_sy, off);
  }
  if (lane == 0 && b_area) {  // (row 0 exists: capacity >= 1)
    atomicMin(&st[0], b_minx); atomicMin(&st[1], b_miny); atomicMax(&st[2], b_maxx); atomicMax(&st[3], b_maxy); atomicAdd(&st[4], (int)b_area);
    atomicAdd(&sm[0], b_sx); atomicAdd(&sm[1], b_sy);
  }
}

__global__ __launch_bounds__(CCL_THREADS) void k_ccl_finish(const CclParams p)
{
  const int frame = blockIdx.y;
  const size_t rows = min((size_t)p.counts[frame], p.capacity);
  int32_t *st = p.stats + (size_t)frame * p.capacity * 5;
  unsigned long long *sm = p.sums + (size_t)frame * p.capacity * 2;
  for (size_t k = (size_t)blockIdx.x * CCL_THREADS + threadIdx.x; k < rows; k += (size_t)gridDim.x * CCL_THREADS) {
    int32_t *s = st + 5 * k;
    double *cen = reinterpret_cast<double *>(sm + 2 * k);
    const int area = s[4];
    if (area == 0) {  // a background without a pixel
      s[0] = 0; s[1] = 0; s[2] = 0; s[3] = 0;
      cen[0] = 0.0; cen[1] = 0.0;
      continue;
    }
    const long long sx = (long long)sm[2 * k], sy = (long long)sm[2 * k + 1];
    s[2] = s[2] - s[0] + 1;
    s[3] = s[3] - s[1] + 1;
    cen[0] = (double)sx / (double)area;
    cen[1] = (double)sy / (double)area;
  }
}

}  // namespace

// One pass on stream s.  capacity == 0: labels and counts only (the three statistics kernels are not launched, p.stats and
// p.sums are not looked at).
hipError_t launch_connected_components(const CclParams &p, hipStream_t s)
{
  if (!p.map || !p.labels || !p.items || !p.counts || (((uintptr_t)p.items | (uintptr_t)p.counts | (uintptr_t)p.labels | p.label_pitch | p.label_frame_stride) & 3u)
      || p.W < 1 || p.H < 1 || p.nframes < 1 || p.nframes > 65535 || p.pitch < (size_t)p.W || p.label_pitch < 4 * (size_t)p.W
      || (unsigned long long)p.H * p.pitch >= (1ull << 32) || (unsigned long long)p.H * p.label_pitch >= (1ull << 32) || (p.connectivity != 4 && p.connectivity != 8)
      || p.tiles_x != (p.W + CCL_TILE_W - 1) / CCL_TILE_W || p.tiles_y != (p.H + CCL_TILE_H - 1) / CCL_TILE_H
      || (long long)p.border_items != (long long)(p.tiles_y - 1) * p.W + (long long)(p.tiles_x - 1) * p.H || p.chunk_rows < 1
      || p.nchunks != (p.H + p.chunk_rows - 1) / p.chunk_rows || (long long)p.total_items != (long long)p.nframes * p.nchunks
      || (p.capacity && (!p.stats || !p.sums || ((uintptr_t)p.stats & 3u) || ((uintptr_t)p.sums & 7u) || p.row_groups < 1)))
    return hipErrorInvalidValue;
  const dim3 block(CCL_THREADS), items_grid((p.total_items + 3) / 4), rows_grid(p.row_groups, p.nframes);
  hipLaunchKernelGGL(k_ccl_local, dim3(p.tiles_x * p.tiles_y, p.nframes), block, 0, s, p);
  if (p.border_items) hipLaunchKernelGGL(k_ccl_merge, dim3((p.border_items + CCL_THREADS - 1) / CCL_THREADS, p.nframes), block, 0, s, p);
  hipLaunchKernelGGL(k_ccl_flatten, items_grid, block, 0, s, p);
  hipLaunchKernelGGL(k_ccl_scan, dim3((p.nframes + 3) / 4), block, 0, s, p);
  hipLaunchKernelGGL(k_ccl_roots, items_grid, block, 0, s, p);
  hipLaunchKernelGGL(k_ccl_number, items_grid, block, 0, s, p);
  if (p.capacity) {
    hipLaunchKernelGGL(k_ccl_rows, rows_grid, block, 0, s, p);
    hipLaunchKernelGGL(k_ccl_stats, items_grid, block, 0, s, p);
    hipLaunchKernelGGL(k_ccl_finish, rows_grid, block, 0, s, p);
  }
  return hipGetLastError();
}

}  // namespace hc
