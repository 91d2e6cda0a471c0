// thin.hip -- the kernels of hc_thinning_device: Zhang-Suen and Guo-Hall thinning of binary maps on bit planes (gfx950, wave64).
//
//   k_thin_pack    u8 map -> bit plane A (a pixel is foreground iff its byte is non-zero); pad bits zero
//   k_thin_step    one sub-iteration: s = 0 reads plane A and writes plane B, s = 1 reads B and writes A
//   k_thin_unpack  plane A -> 0 / 255 bytes of the output view, and the status pair of each frame
// Layout (canny_params.h): a plane row is thin_row_words(W) dwords, bit i of word j = column 32 j + i.  In k_thin_step a lane
// holds one dword of a row and a wave a panel of 64 words; a work item is (frame, panel, tile of THIN_TILE_ROWS rows), one per
// wave.  The wave streams down its tile with a window of three rows in registers, each row as three planes: the row itself, its
// west neighbours ((w << 1) | the left lane's bit 31) and its east neighbours, the neighbouring lane's word by DPP and, at the
// first and last lane of a panel, the adjacent panel's word from memory (or zero at the frame's edge).  The eight neighbour planes
// P2 .. P9 feed bit-sliced logic (thin_removed, canny_params.h), 32 pixels per instruction: no per-pixel branch, no LDS, no bytes.
// Planes are ping-pong: every decision of a sub-iteration is taken on the source plane, which no item writes, so tiles need no
// order and share nothing but the halo rows they read.  Pad bits stay zero (a sub-iteration only clears bits), so no column is
// tested against W; rows outside the frame enter the window as zeros, wave-uniformly.
// Per-frame stop: every wave first reads the frame's removal word of the previous iteration and exits if it is zero (iteration
// 1: no test); a wave that cleared pixels adds their number to the frame's word of this iteration with one atomic add.  Integer
// sums: the table, and with it which launches work, is a function of the map alone.
#include "canny_device.h"

namespace hc {

namespace {

// the segment of 256 columns a wave of k_thin_pack / k_thin_unpack works on
struct SegItem { int frame, row, seg; bool valid; };
static __device__ __forceinline__ SegItem seg_item(int nframes, int H, int segs)
{
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long total = (long long)nframes * H * segs;
  SegItem it;
  it.valid = wave < total;
  it.seg = (int)(wave % segs);
  it.row = (int)((wave / segs) % H);
  it.frame = (int)(wave / ((long long)segs * H));
  return it;
}

}  // namespace

__global__ __launch_bounds__(256) void k_thin_pack(const ThinPackParams p)
{
  const SegItem it = seg_item(p.nframes, p.H, p.segs);
  if (!it.valid) return;
  const int lane = threadIdx.x & 63;
  const int c0 = it.seg * THIN_SEG_PX + lane * 4;
  const uint8_t *rowp = p.map + (size_t)it.frame * p.frame_stride + (size_t)it.row * p.pitch;
  u32 nib = 0;
  if (p.in_aligned && c0 + 3 < p.W) {
    const u32 v = *reinterpret_cast<const u32 *>(rowp + c0);
    nib = ((v & 0xFFu) ? 1u : 0u) | ((v & 0xFF00u) ? 2u : 0u) | ((v & 0xFF0000u) ? 4u : 0u) | ((v & 0xFF000000u) ? 8u : 0u);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < p.W) nib |= rowp[c0 + k] ? (1u << k) : 0u;
  }
  // 8 lanes' nibbles -> one word, in the lanes 0, 8, 16, ..: pairs, fours, eights (zeros enter above lane 63)
  const u32 b = nib | (from_lane_above(nib) << 4);
  const u32 h = b | (from_lane_above(from_lane_above(b)) << 8);
  const u32 w = h | (from_lane_above(from_lane_above(from_lane_above(from_lane_above(h)))) << 16);
  const int word = it.seg * (THIN_SEG_PX / 32) + (lane >> 3);
  if (!(lane & 7) && word < p.row_words) p.plane_a[(size_t)it.frame * p.plane_words + (size_t)it.row * p.row_words + word] = w;
}

template <int METHOD, int S>
__global__ __launch_bounds__(256) void k_thin_step(const ThinStepParams p, const int iteration)
{
  const int lane = threadIdx.x & 63;
  const int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (item >= p.total_items) return;
  const int tile = item % p.ntiles;
  const int panel = (item / p.ntiles) % p.npanels;
  const int frame = item / (p.ntiles * p.npanels);
  u32 *const rem = p.removed + (size_t)frame * p.table_words;
  if (iteration > 1 && rem[iteration - 1] == 0) return;  // the frame reached its fixed point (wave-uniform: one scalar load)

  const u32 *const src = (S == 0 ? p.plane_a : p.plane_b) + (size_t)frame * p.plane_words;
  u32 *const dst = (S == 0 ? p.plane_b : p.plane_a) + (size_t)frame * p.plane_words;
  const int RW = p.row_words, H = p.H;
  const int wi = panel * THIN_PANEL_WORDS + lane;
  const bool act = wi < RW;
  const int r0 = tile * THIN_TILE_ROWS, rend = min(r0 + THIN_TILE_ROWS, H);
  const int last = min(rend, H - 1);  // the last source row this item reads: its lower halo row, where the frame has one
  // the adjacent panels' words: lane 0 reads the word left of the panel, lane 63 the word right of it (wave-uniformly none in a
  // frame of one panel)
  const bool panels = p.npanels > 1;
  const int hw = lane == 0 ? wi - 1 : wi + 1;
  const bool halo = panels && (lane == 0 || lane == 63) && hw >= 0 && hw < RW;

  struct Raw { u32 c, h; };
  auto load = [&](int r) -> Raw {
    Raw q{ 0u, 0u };
    if (r < 0 || r > last) return q;  // wave-uniform: rows outside the frame (or this item's reach) are zeros
    const u32 *rp = src + (u32)r * (u32)RW;
    if (act) q.c = rp[wi];
    if (panels && halo) q.h = rp[hw];
    return q;
  };
  auto make = [&](const Raw &q) -> ThinRow {
    u32 left = from_lane_below(q.c), right = from_lane_above(q.c);
    if (panels) {
      left = lane == 0 ? q.h : left;
      right = lane == 63 ? q.h : right;
    }
    return ThinRow{ q.c, (q.c << 1) | (left >> 31), (q.c >> 1) | (right << 31) };
  };

  ThinRow N = make(load(r0 - 1)), C = make(load(r0));
  Raw q1 = load(r0 + 1), q2 = load(r0 + 2);
  u32 cleared = 0;
  for (int r = r0; r < rend; ++r) {
    const ThinRow S_ = make(q1);
    q1 = q2;
    q2 = load(r + 3);
    const u32 gone = thin_removed<METHOD, S>(N, C, S_);
    if (act) dst[(u32)r * (u32)RW + wi] = C.c & ~gone;
    cleared += __builtin_popcount(gone);
    N = C;
    C = S_;
  }
  if (__builtin_amdgcn_ballot_w64(cleared != 0) == 0) return;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cleared += __shfl_xor(cleared, d, 64);
  if (lane == 0) atomicAdd(&rem[iteration], cleared);
}

__global__ __launch_bounds__(256) void k_thin_unpack(const ThinUnpackParams p)
{
  const SegItem it = seg_item(p.nframes, p.H, p.segs);
  if (!it.valid) return;
  const int lane = threadIdx.x & 63;
  const int c0 = it.seg * THIN_SEG_PX + lane * 4;
  const int word = it.seg * (THIN_SEG_PX / 32) + (lane >> 3);
  if (c0 < p.W) {
    const u32 w = p.plane_a[(size_t)it.frame * p.plane_words + (size_t)it.row * p.row_words + word];
    const u32 bytes = nibble_to_bytes((w >> (4 * (lane & 7))) & 0xFu);
    uint8_t *q = p.out + (size_t)it.frame * p.out_frame_stride + (size_t)it.row * p.out_pitch + c0;
    if (p.out_aligned && c0 + 3 < p.W) *reinterpret_cast<u32 *>(q) = bytes;
    else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k < p.W) q[k] = (uint8_t)(bytes >> (8 * k));
    }
  }
  // the frame's first wave: the iterations that removed a pixel (a prefix of the table's words 1 .. max_iterations), and
  // whether one of them removed none
  if (p.status && it.row == 0 && it.seg == 0) {
    const u32 *rem = p.removed + (size_t)it.frame * p.table_words;
    u32 n = 0;
    for (int k0 = 1; k0 <= p.max_iterations; k0 += 64) {
      const int k = k0 + lane;
      n += (u32)__builtin_popcountll(__builtin_amdgcn_ballot_w64(k <= p.max_iterations && rem[k] != 0));
    }
    if (lane < 2) p.status[2 * (size_t)it.frame + lane] = lane == 0 ? n : (n < (u32)p.max_iterations ? 1u : 0u);
  }
}

hipError_t launch_thin_pack(const ThinPackParams &p, hipStream_t s)
{
  const long long total = (long long)p.nframes * p.H * p.segs;
  if (p.W < 1 || p.H < 1 || p.nframes < 1 || !p.map || !p.plane_a || p.pitch < (size_t)p.W || p.row_words != thin_row_words(p.W) || p.segs != thin_segs(p.W)
      || p.plane_words != (size_t)p.H * p.row_words || total > 0x7FFFFFF0ll * 4)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_thin_pack, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_thin_step(const ThinStepParams &p, int sub, int iteration, hipStream_t s)
{
  if (p.H < 1 || p.nframes < 1 || p.row_words < 1 || !p.plane_a || !p.plane_b || !p.removed || p.plane_words != (size_t)p.H * p.row_words
      || p.npanels != (p.row_words + THIN_PANEL_WORDS - 1) / THIN_PANEL_WORDS || p.ntiles != thin_tiles(p.H)
      || (long long)p.total_items != (long long)p.nframes * p.npanels * p.ntiles || iteration < 1 || iteration >= p.table_words || (sub != 0 && sub != 1)
      || (p.method != THIN_ZHANGSUEN && p.method != THIN_GUOHALL) || p.plane_words > 0x3FFFFFFFull)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((p.total_items + 3) / 4)), block(256);
  if (p.method == THIN_ZHANGSUEN) {
    if (sub == 0) hipLaunchKernelGGL((k_thin_step<THIN_ZHANGSUEN, 0>), grid, block, 0, s, p, iteration);
    else hipLaunchKernelGGL((k_thin_step<THIN_ZHANGSUEN, 1>), grid, block, 0, s, p, iteration);
  } else {
    if (sub == 0) hipLaunchKernelGGL((k_thin_step<THIN_GUOHALL, 0>), grid, block, 0, s, p, iteration);
    else hipLaunchKernelGGL((k_thin_step<THIN_GUOHALL, 1>), grid, block, 0, s, p, iteration);
  }
  return hipGetLastError();
}

hipError_t launch_thin_unpack(const ThinUnpackParams &p, hipStream_t s)
{
  const long long total = (long long)p.nframes * p.H * p.segs;
  if (p.W < 1 || p.H < 1 || p.nframes < 1 || !p.out || !p.plane_a || !p.removed || p.out_pitch < (size_t)p.W || p.row_words != thin_row_words(p.W)
      || p.segs != thin_segs(p.W) || p.plane_words != (size_t)p.H * p.row_words || p.max_iterations < 1 || p.table_words != p.max_iterations + 1
      || total > 0x7FFFFFF0ll * 4)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_thin_unpack, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace hc
