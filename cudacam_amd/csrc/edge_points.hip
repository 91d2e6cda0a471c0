// edge_points.hip -- the non-zero pixels of u8 maps as coordinate lists in raster order and their number, per frame
// (hc_edge_points_device: cv::findNonZero / cv::countNonZero on the device).
//
//   k_edge_count  a work item is (frame, chunk of rows) and belongs to one wave: the number of non-zero bytes of its rows ->
//                 items[frame][chunk].  The row reader is k_hist256's (stats.hip): the dwords that lie whole inside
//                 [row, row + W) as dwords, four in flight, the up to three bytes before and after them bytewise, so no byte
//                 outside the row is read at any alignment.  One lane's plain store per item, no atomics.
//   k_edge_scan   one wave per frame: exclusive prefix sum over the frame's items (64 per trip, with a carry), in place -- an
//                 item's entry becomes the index of its first point in the frame's list -- and the total -> counts[frame].
//   k_edge_emit   the work split of k_edge_count again: every item writes its points from its offset on, while the index is
//                 below `capacity`.
//
// The order.  Inside a row k_edge_emit visits the head bytes, then the body in trips of 64 consecutive dwords (lane l holds
// dword 64 k + l of trip k), then the tail bytes.  Inside a trip a point's index is the running offset + the non-zero bytes
// of the lanes below (ballot of every byte position, v_mbcnt of each) + the non-zero bytes below it in its own dword: lanes
// ascend with the column, bytes with the column inside a lane, trips and rows follow each other in the wave's own loop, and
// the items of a frame start where the scan puts them -- raster order, whatever the split.  The running offset comes from
// population counts of ballots only, so it is wave-uniform and lives in SGPRs; a trip whose dwords are all zero costs its load
// and one ballot (four trips are loaded together and skipped together when all are empty: on edge maps most are).
// The wave prefix is the mbcnt form: four ballots and eight v_mbcnt per non-empty trip, no cross-lane data movement; a DPP
// scan of the lanes' byte counts (six dependent row shifts / broadcasts on wave64) has not been built for comparison.
#include "canny_device.h"

namespace hc {

namespace {

// bit 7 of every non-zero byte of d
static __device__ __forceinline__ u32 nonzero_bytes(u32 d) { return (((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u; }

struct RowSplit { int head, nd, tail; };  // bytes before the first aligned dword, whole dwords inside the row, bytes after them
static __device__ __forceinline__ RowSplit split_row(const uint8_t *rp, int nb)
{
  RowSplit s;
  s.head = min((int)((0u - (u32)(uintptr_t)rp) & 3u), nb);
  s.nd = (nb - s.head) >> 2;
  s.tail = nb - s.head - 4 * s.nd;
  return s;
}

__global__ __launch_bounds__(256) void k_edge_count(const EdgePointsParams p)
{
  const int lane = threadIdx.x & 63;
  const int item = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (int)(threadIdx.x >> 6));
  if (item >= p.total_items) return;
  const int chunk = item % p.nchunks;
  const int frame = item / p.nchunks;
  const int r0 = chunk * p.chunk_rows, rend = min(r0 + p.chunk_rows, p.H);
  const uint8_t *fbase = p.map + (size_t)frame * p.frame_stride;
  u32 n = 0;
  for (int row = r0; row < rend; ++row) {  // everything but `lane` is wave-uniform
    const uint8_t *rp = fbase + (size_t)row * p.pitch;
    const RowSplit s = split_row(rp, p.W);
    if (lane < s.head) n += rp[lane] != 0;
    if (lane >= 32 && lane - 32 < s.tail) n += rp[s.head + 4 * s.nd + (lane - 32)] != 0;
    const u32 *body = reinterpret_cast<const u32 *>(rp + s.head);
    int i = lane;
    for (; i + 192 < s.nd; i += 256) {
      const u32 d0 = body[i], d1 = body[i + 64], d2 = body[i + 128], d3 = body[i + 192];
      n += __popc(nonzero_bytes(d0)) + __popc(nonzero_bytes(d1)) + __popc(nonzero_bytes(d2)) + __popc(nonzero_bytes(d3));
    }
    for (; i < s.nd; i += 64) n += __popc(nonzero_bytes(body[i]));
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off);
  if (lane == 0) p.items[item] = n;
}

__global__ __launch_bounds__(256) void k_edge_scan(const EdgePointsParams p)
{
  const int lane = threadIdx.x & 63;
  const int frame = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (frame >= p.nframes) return;
  u32 *it = p.items + (size_t)frame * p.nchunks;
  u32 carry = 0;  // points of the chunks before this trip (a frame holds fewer than 2^32 pixels)
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
  if (lane == 0) p.counts[frame] = carry;
}

__global__ __launch_bounds__(256) void k_edge_emit(const EdgePointsParams p)
{
  const int lane = threadIdx.x & 63;
  const int item = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (int)(threadIdx.x >> 6));
  if (item >= p.total_items) return;
  const int chunk = item % p.nchunks;
  const int frame = item / p.nchunks;
  const u32 cap = (u32)min(p.capacity, (size_t)0xFFFFFFFFu);  // (indices stay below the frame's pixel count < 2^32)
  u32 off = (u32)__builtin_amdgcn_readfirstlane((int)p.items[item]);  // index of the next point in the frame's list: wave-uniform
  if (off >= cap) return;
  const int r0 = chunk * p.chunk_rows, rend = min(r0 + p.chunk_rows, p.H);
  const uint8_t *fbase = p.map + (size_t)frame * p.frame_stride;
  int2 *out = reinterpret_cast<int2 *>(p.points) + (size_t)frame * p.capacity;
  for (int row = r0; row < rend; ++row) {
    const uint8_t *rp = fbase + (size_t)row * p.pitch;
    const RowSplit s = split_row(rp, p.W);
    // lanes 0..2: one head / tail byte each, at column x0 + lane
    auto emit_bytes = [&](u32 b, int x0) {
      const u64 m = __ballot(b != 0);
      if (m == 0) return;
      const u32 slot = off + mbcnt64(m);
      if (b != 0 && slot < cap) out[slot] = make_int2(x0 + lane, row);
      off += (u32)__popcll(m);
    };
    // one trip: the lane's dword d holds columns x0 .. x0 + 3
    auto emit_dword = [&](u32 d, int x0) {
      const u32 nz = nonzero_bytes(d);
      if (__ballot(nz != 0) == 0) return;
      u32 slot = off;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u64 m = __ballot((nz >> (8 * j + 7)) & 1u);
        slot += mbcnt64(m);
        off += (u32)__popcll(m);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((nz >> (8 * j + 7)) & 1u) {
          if (slot < cap) out[slot] = make_int2(x0 + j, row);
          ++slot;
        }
    };
    const u32 hb = lane < s.head ? rp[lane] : 0u;
    const u32 tb = lane < s.tail ? rp[s.head + 4 * s.nd + lane] : 0u;
    emit_bytes(hb, 0);
    if (off >= cap) return;
    const u32 *body = reinterpret_cast<const u32 *>(rp + s.head);
    for (int i0 = 0; i0 < s.nd; i0 += 256) {  // four trips in flight
      const int i = i0 + lane;
      const u32 d0 = i < s.nd ? body[i] : 0u, d1 = i + 64 < s.nd ? body[i + 64] : 0u;
      const u32 d2 = i + 128 < s.nd ? body[i + 128] : 0u, d3 = i + 192 < s.nd ? body[i + 192] : 0u;
      if (__ballot((d0 | d1 | d2 | d3) != 0) == 0) continue;
      const int x0 = s.head + 4 * i;
      emit_dword(d0, x0);
      emit_dword(d1, x0 + 256);
      emit_dword(d2, x0 + 512);
      emit_dword(d3, x0 + 768);
      if (off >= cap) return;
    }
    emit_bytes(tb, s.head + 4 * s.nd);
    if (off >= cap) return;
  }
}

}  // namespace

// The three launches on stream s.  capacity == 0: counts only (k_edge_emit is not launched, p.points is not looked at).
hipError_t launch_edge_points(const EdgePointsParams &p, hipStream_t s)
{
  if (!p.map || !p.items || !p.counts || (((uintptr_t)p.items | (uintptr_t)p.counts) & 3u) || p.W < 1 || p.H < 1 || p.nframes < 1 || p.pitch < (size_t)p.W
      || (unsigned long long)p.H * p.pitch >= (1ull << 32) || p.chunk_rows < 1 || p.nchunks != (p.H + p.chunk_rows - 1) / p.chunk_rows
      || (long long)p.total_items != (long long)p.nframes * p.nchunks || (p.capacity && (!p.points || ((uintptr_t)p.points & 7u))))
    return hipErrorInvalidValue;
  const dim3 items_grid((p.total_items + 3) / 4), block(256);
  hipLaunchKernelGGL(k_edge_count, items_grid, block, 0, s, p);
  hipLaunchKernelGGL(k_edge_scan, dim3((p.nframes + 3) / 4), block, 0, s, p);
  if (p.capacity) hipLaunchKernelGGL(k_edge_emit, items_grid, block, 0, s, p);
  return hipGetLastError();
}

}  // namespace hc
