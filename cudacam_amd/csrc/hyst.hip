// hyst.hip -- the edge hysteresis of the hipcanny hot path on the bit planes (gfx950, CDNA4, wave64): k_pack (tri-state
// u8 map -> planes, the entry of hc_hysteresis_device), k_hyst (one launch of the fixpoint iteration; writes or patches
// the 0/255 u8 edge map as it goes), k_hyst_loop (all launches of a small run in one) and their launchers.  Which shape
// and which schedule a run gets is the planner's business (host_plan.h); the shapes themselves are HYST_SHAPES
// (canny_params.h).
#include "canny_device.h"
#include <algorithm>
#include <type_traits>
#include <utility>

namespace hc {

// =================================================================================================
// k_pack: tri-state u8 map (0 / 128 / 255) -> bit planes (entry of hc_hysteresis_device)
// =================================================================================================
__global__ __launch_bounds__(256) void k_pack(const PackParams p)
{
  const int lane = threadIdx.x & 63;
  const int segs = (p.W + 255) / 256;  // 256 px (64 lanes x 4) per wave
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long total = (long long)p.nframes * p.H * segs;
  if (wave >= total) return;
  const int seg = (int)(wave % segs);
  const int row = (int)((wave / segs) % p.H);
  const int frame = (int)(wave / ((long long)segs * p.H));
  const int c0 = seg * 256 + lane * 4;
  const uint8_t *rowp = p.in + (size_t)frame * p.in_frame_stride + (size_t)row * p.in_pitch;
  u32 nib = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const u32 v = (c0 + k < p.W) ? rowp[c0 + k] : 0u;
    nib |= (v == 255u) ? (1u << k) : 0u;
    nib |= (v >= 128u) ? (0x100u << k) : 0u;
  }
  const u32 w = nib | (from_lane_above(nib) << 4);
  const size_t off = ((size_t)frame * p.H + row) * p.RD * 4 + (size_t)seg * 32 + (size_t)(lane >> 1);
  if (!(lane & 1) && (size_t)seg * 32 + (size_t)(lane >> 1) < (size_t)p.RD * 4) {
    reinterpret_cast<uint8_t *>(p.sbits)[off] = (uint8_t)w;
    reinterpret_cast<uint8_t *>(p.cbits)[off] = (uint8_t)(w >> 8);
  }
}

hipError_t launch_pack(const PackParams &p, hipStream_t s)
{
  const long long total = (long long)p.nframes * p.H * ((p.W + 255) / 256);
  hipLaunchKernelGGL(k_pack, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, p);
  return hipGetLastError();
}

// =================================================================================================
// k_hyst: edge hysteresis on the bit planes, by row sweeps with carry look-ahead
// =================================================================================================
// A candidate with a strong 8-neighbour becomes strong, to the fixpoint (cannyEdgeD.cu:342-352,
// launch loop cannyEdgeH.cu:307-324).  Work item = (frame, tile of tile_rows rows), one per wave;
// a whole bit-plane row lives in the wave (lane l holds dwords l*NW .. l*NW+NW-1).  The wave sweeps
// its rows downwards, then upwards: row r takes the strong bits of the previous row dilated by one
// column each way, ANDs with its candidates, and then FILLS every candidate run touched by a strong
// bit along the whole row at once: adding the seeds to the candidate word ripples a carry through
// each run ((c + s) ^ c marks the bits above the seed), lanes are chained by a carry look-ahead over
// the per-lane generate/propagate ballots (one 64-bit scalar add), and the bit-reversed pass fills
// the other direction.  One down+up pair settles every path that is monotone in the row index, so
// a tile converges in a few sweeps however long its chains are -- unlike pixel-per-iteration
// propagation (the reference moves one 30x30 tile per launch).  Tiles exchange boundary rows across
// launches; per-tile change flags let later launches touch only the tiles next to a change, and the
// flag word of the last queued launch tells the host whether the fixpoint was reached.

// How a launch finds the tiles with work, and what it leaves for the next one (HystParams::lists and iter: hyst_mode).
enum HystMode : int {
  // Every launch starts a workgroup per tile, and a tile looks at the reason word its neighbours left it in the previous
  // launch (p.wl_reason); launch index at run time (p.iter).
  HYST_PER_TILE = 0,
  // Launch 0 of the worklist scheme -- every tile, every row open; tiles that change a boundary append the neighbours
  // that look at it to the next launch's list.
  HYST_LIST_FIRST = 1,
  // A later launch of the worklist scheme; the tile is on the list because a neighbour above / below / beside changed the
  // row or column it looks at (top / bot / side).
  HYST_LIST_LATE = 2,
  // As HYST_PER_TILE, but the neighbours also go on the next launch's list: the launch between per-tile launches and list
  // launches of a run that starts with the former and ends with the latter.
  HYST_PER_TILE_TO_LIST = 3,
};
static inline HystMode hyst_mode(int lists, int iter)
{
  return lists == 2 ? HYST_PER_TILE_TO_LIST : lists != 1 ? HYST_PER_TILE : iter > 0 ? HYST_LIST_LATE : HYST_LIST_FIRST;
}

template <int NW>
struct RowBits {
  u32 w[NW];
};

template <int NW>
static __device__ __forceinline__ RowBits<NW> row_load(const u32 *plane_row, int lane, int RD)
{
  RowBits<NW> r;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int d = lane * NW + i;
    r.w[i] = d < RD ? plane_row[d] : 0u;
  }
  return r;
}

// fill every run of `c` that contains a bit of `s` (s subset of c), over the whole row
template <int NW>
static __device__ __forceinline__ RowBits<NW> row_fill(const RowBits<NW> &c, const RowBits<NW> &s)
{
  RowBits<NW> out;
  // towards higher columns
  {
    u32 t[NW];
    u32 carry = 0;
    bool allones = true;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const u64 x = (u64)c.w[i] + s.w[i] + carry;
      t[i] = (u32)x;
      carry = (u32)(x >> 32);
      allones = allones && (t[i] == 0xFFFFFFFFu);
    }
    const u64 G = __ballot(carry != 0), P = __ballot(allones);
    const u64 A = G | P;
    const u64 cin = (A + G) ^ A ^ G;  // carry into each lane (look-ahead by one scalar add)
    carry = __builtin_amdgcn_inverse_ballot_w64(cin) ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const u64 x = (u64)c.w[i] + s.w[i] + carry;
      carry = (u32)(x >> 32);
      out.w[i] = (((u32)x ^ c.w[i]) & c.w[i]) | s.w[i];
    }
  }
  // towards lower columns: the same on the bit-reversed row (lane order reversed in the look-ahead)
  {
    u32 rc[NW], rs[NW], t[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      rc[i] = __builtin_bitreverse32(c.w[NW - 1 - i]);
      rs[i] = __builtin_bitreverse32(s.w[NW - 1 - i]);
    }
    u32 carry = 0;
    bool allones = true;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const u64 x = (u64)rc[i] + rs[i] + carry;
      t[i] = (u32)x;
      carry = (u32)(x >> 32);
      allones = allones && (t[i] == 0xFFFFFFFFu);
    }
    const u64 G = __builtin_bitreverse64(__ballot(carry != 0)), P = __builtin_bitreverse64(__ballot(allones));
    const u64 A = G | P;
    const u64 cin = __builtin_bitreverse64((A + G) ^ A ^ G);
    carry = __builtin_amdgcn_inverse_ballot_w64(cin) ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const u64 x = (u64)rc[i] + rs[i] + carry;
      carry = (u32)(x >> 32);
      const u32 f = (((u32)x ^ rc[i]) & rc[i]);
      out.w[NW - 1 - i] |= __builtin_bitreverse32(f);
    }
  }
  return out;
}

// strong bits of the neighbouring row, dilated by one column each way
template <int NW>
static __device__ __forceinline__ RowBits<NW> row_dilate(const RowBits<NW> &p)
{
  RowBits<NW> d;
  const u32 below = from_lane_below(p.w[NW - 1]);  // previous lane's last dword
  const u32 above = from_lane_above(p.w[0]);       // next lane's first dword
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const u32 lo = i == 0 ? below : p.w[i - 1];
    const u32 hi = i == NW - 1 ? above : p.w[i + 1];
    d.w[i] = p.w[i] | __builtin_amdgcn_alignbit(p.w[i], lo, 31) | __builtin_amdgcn_alignbit(hi, p.w[i], 1);
  }
  return d;
}

// Whole rows of a wave's tile to the 0/255 map, straight from the row registers: the rows in `rows` (bit r = row r of the tile,
// wave-uniform; `srow` = the wave's strong rows, this lane's dword of each; out0 = row 0 of the tile in the frame's map), the
// columns of the panel that starts at dword pcol, below W.  Two passes of 64 groups of 16 pixels, a group per lane and store.
// Exactly the bytes [32 pcol, min(W, 32 (pcol + ROWW))) of each row are written.
template <int ROWW, class RowVec>
static __device__ __forceinline__ void expand_rows(const RowVec &srow, u64 rows, uint8_t *out0, size_t pitch, int pcol, int W, bool a16, int lane)
{
  for (u64 m = rows; m != 0; m &= m - 1) {
    const int r = __builtin_ctzll(m);
    const u32 rowv = srow[r];
    uint8_t *orow = out0 + (size_t)r * pitch;
    for (int pass = 0; pass * 1024 < ROWW * 32 && pcol * 32 + pass * 1024 < W; ++pass) {
      // this lane writes px [32*pcol + 1024*pass + 16*lane, +16): half-word 64*pass + lane of the panel row
      const u32 x = __shfl(rowv, 32 * pass + (lane >> 1));  // before any lane drops out: the permute only sees active lanes
      const u32 b = (x >> (16 * (lane & 1))) & 0xFFFFu;
      const int c0 = pcol * 32 + pass * 1024 + lane * 16;
      if (c0 + 15 >= W) continue;  // whole 16-pixel groups here; the ragged last group of a row below
      u32 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = nibble_to_bytes((b >> (4 * k)) & 0xFu);
      uint8_t *dst = orow + c0;
      if (a16) {
        // (the pointer goes through an empty asm: seeing two branches that store the same bytes, the optimizer otherwise
        //  merges them into the four dword stores -- twice the store instructions)
        uint8_t *d16 = dst;
        asm volatile("" : "+v"(d16));
        *reinterpret_cast<uint4 *>(d16) = make_uint4(v[0], v[1], v[2], v[3]);
      } else
#pragma unroll
        for (int k = 0; k < 4; ++k) reinterpret_cast<u32 *>(dst)[k] = v[k];
    }
  }
  // Widths that are not a multiple of 16: the last W % 16 pixels of every row, a byte per lane, in a loop of their own
  // (inside the loop above, the byte-wise tail -- unrolled 16 times under 16 exec masks -- cost the kernel an SGPR
  // spill, i.e. an 81st VGPR, and as a plain loop it made the compiler split the hot loop: 0.94 instead of 0.76 ms
  // for launch 0 of 1024 frames in plain mode)
  const int ragged = W & 15, cl = W - ragged;  // first column of the ragged group
  if (ragged != 0 && cl >= pcol * 32 && cl < (pcol + ROWW) * 32) {
    const int hw = (cl - pcol * 32) >> 4;  // its half-word in the panel row: dword hw / 2 is held by lane hw / 2
    for (u64 m = rows; m != 0; m &= m - 1) {
      const int r = __builtin_ctzll(m);
      const u32 x = __shfl(srow[r], hw >> 1);
      const u32 b = (x >> (16 * (hw & 1))) & 0xFFFFu;
      if (lane < ragged) (out0 + (size_t)r * pitch + cl)[lane] = ((b >> lane) & 1u) ? (uint8_t)255 : (uint8_t)0;
    }
  }
}

// Workgroup tile = WAVES waves x TR rows.  Every wave keeps its TR rows of both planes in REGISTERS
// (lane l holds dwords l*NW.. of each row; rows are picked with a wave-uniform index, which the
// compiler turns into VGPR-indexed moves); LDS only carries the rows neighbours look at.
// (the shapes: HYST_SHAPES; which one a run gets: hyst_tile_geometry, both canny_params.h)

// PANELS: the frame is wider than one 2048-column panel (tiles then also have left / right neighbours); the common
// narrower case is compiled without that code.
// One workgroup tile, gtile = frame * tiles per frame + tile.  MODE: a HystMode.
template <int NW, int TR, int WAVES, bool PANELS, int MODE>
static __device__ __forceinline__ void hyst_tile(const HystParams &p, int gtile, bool top, bool bot, bool side)
{
  constexpr bool WORDS_IN = MODE == HYST_PER_TILE || MODE == HYST_PER_TILE_TO_LIST;  // the tile finds its reason in its word (a workgroup per tile)
  const bool LATE = WORDS_IN ? p.iter > 0 : MODE == HYST_LIST_LATE;
  static_assert(NW == 1, "frames wider than one panel are tiled in column panels; a lane holds one dword per row");
  static_assert((TR & (TR - 1)) == 0, "row indices are wrapped with TR - 1");
  constexpr int ROWW = 64 * NW;  // dwords per row
  constexpr int BR = WAVES * TR;
  constexpr int XQ_CAP = 256;  // a row adds up to 128 groups to a queue holding fewer than 64
  __shared__ u32 edge[(2 * WAVES + 2) * ROWW];  // per wave: first and last row of S; then the two halo rows
  __shared__ u32 bchg[24];
  __shared__ u32 xqueue[WAVES * XQ_CAP];
  const int lane = threadIdx.x & 63, wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // tiles are 2-D: row tile bt x column panel pn (a panel = ROWW dwords = 2048 columns; frames up to 2048
  // columns have one panel).  A wave always holds one dword per lane and row, whatever the frame width.
  const int NP = PANELS ? p.npanels : 1, ntile = p.nrtiles * NP;
  const int tile = gtile % ntile, frame = gtile / ntile;
  const int bt = tile / NP, pn = tile % NP;
  const int H = p.H, RD = p.RD;
  const int pcol = pn * ROWW;                          // first dword of this panel in a plane row
  const int b0 = bt * BR, nb = min(H, b0 + BR) - b0;  // rows of this workgroup tile
  if (WORDS_IN && LATE) {
    // work only if a neighbouring tile changed the row / column / corner this tile looks at: it left its reason in this
    // tile's word of the launch's parity (one load; cleared for the launch after next)
    u32 *reason = p.wl_reason + (size_t)(p.iter & 1) * p.wl_stride;
    const u32 why = (u32)__builtin_amdgcn_readfirstlane((int)reason[gtile]);
    top = (why & 1u) != 0; bot = (why & 2u) != 0; side = (why & 4u) != 0;
    if (why != 0) {
      __syncthreads();  // (uniform branch) everyone has the reason before it is cleared
      if (threadIdx.x == 0) {
        reason[gtile] = 0;
        if (PANELS) atomicAdd(&p.wl_count[p.iter], 1u);  // wide frames: how many tiles this launch visits (the host picks worklists or this form by it)
      }
    }
  }
  if (LATE) {
    if (!top && !bot && !side) return;  // uniform for the workgroup
    // A neighbour's boundary row changed somewhere -- but does a new bit reach a candidate of this tile?  Only
    // then can anything change here (the tile is at its own fixpoint).  Checked on the two boundary rows alone
    // (4 row loads) before the 2 x TR rows per wave are fetched: most tiles leave here in launches >= 1.
    if (!PANELS && !side) {
      u32 *S0 = p.sbits + (size_t)frame * H * RD;
      const u32 *C0 = p.cbits + (size_t)frame * H * RD;
      bool hit = false;
      auto reaches = [&](int halo_row, int my_row) {
        const RowBits<NW> hv = row_load<NW>(S0 + (size_t)halo_row * RD, lane, RD);
        const RowBits<NW> sv = row_load<NW>(S0 + (size_t)my_row * RD, lane, RD), cv = row_load<NW>(C0 + (size_t)my_row * RD, lane, RD);
        const RowBits<NW> d = row_dilate<NW>(hv);
        bool h = false;
#pragma unroll
        for (int j = 0; j < NW; ++j) h = h || ((cv.w[j] & d.w[j] & ~sv.w[j]) != 0);
        return __ballot(h) != 0;
      };
      if (top && wib == 0) hit = reaches(b0 - 1, b0);
      if (bot && wib == WAVES - 1) hit = reaches(b0 + nb, b0 + nb - 1) || hit;
      if (threadIdx.x == 0) bchg[20] = 0;
      __syncthreads();
      if (hit && lane == 0) atomicOr(&bchg[20], 1u);
      __syncthreads();
      if (__builtin_amdgcn_readfirstlane(bchg[20]) == 0) return;
    }
  }
  // this wave's rows inside the workgroup tile
  const int w0 = min(wib * TR, nb), n = min((wib + 1) * TR, nb) - w0;
  const bool owns_last = n > 0 && w0 + n == nb;
  const u64 all_rows = n >= 64 ? ~0ull : ((1ull << n) - 1);
  u64 dirty;  // bit r = row b0 + w0 + r needs (re)evaluation
  if (LATE) dirty = side ? all_rows : (((top && w0 == 0 && n > 0) ? 1ull : 0ull) | ((bot && owns_last) ? (1ull << (n - 1)) : 0ull));
  else dirty = all_rows;
  dirty = uniform64(dirty);
  u64 unfilled = p.first_pass ? all_rows : 0ull;  // rows not yet closed under the in-row fill

  u32 *S = p.sbits + (size_t)frame * H * RD;
  const u32 *C = p.cbits + (size_t)frame * H * RD;
  // the wave's rows: straight from HBM into registers, all loads in flight at once
  // (ext_vector types: the compiler keeps them in VGPRs and indexes them with s_set_gpr_idx;
  //  plain arrays with dynamic stores would be demoted to scratch)
  typedef u32 RowVec __attribute__((ext_vector_type(TR)));
  RowVec cr[NW], sr[NW];
  // (a panel is always 64 whole dwords wide -- launch_hyst: RD % 64 == 0 -- so only the row count limits the loads)
  if (n == TR) {  // all but the last wave tile of a frame: no per-row test
#pragma unroll
    for (int i = 0; i < TR; ++i) {
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        const size_t off = (size_t)(b0 + w0 + i) * RD + pcol + lane * NW + j;
        cr[j][i] = C[off];
        sr[j][i] = S[off];
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < TR; ++i) {
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        const bool ok = i < n;  // wave-uniform
        const size_t off = (size_t)(b0 + w0 + i) * RD + pcol + lane * NW + j;
        cr[j][i] = ok ? C[off] : 0u;
        sr[j][i] = ok ? S[off] : 0u;
      }
    }
  }
  u32 *my_first = edge + (2 * wib) * ROWW, *my_last = edge + (2 * wib + 1) * ROWW;
  u32 *halo_top = edge + (2 * WAVES) * ROWW, *halo_bot = edge + (2 * WAVES + 1) * ROWW;
  auto publish = [&](u32 *dst, int r) {
#pragma unroll
    for (int j = 0; j < NW; ++j) dst[lane * NW + j] = sr[j][r];
  };
  if (n > 0) {
    publish(my_first, 0);
    publish(my_last, n - 1);
  }
  if (wib == 0 || owns_last) {  // rows just outside the tile (owned by the neighbouring workgroups, or outside the frame)
    const int gr = wib == 0 ? b0 - 1 : b0 + nb;
    RowBits<NW> v;
#pragma unroll
    for (int j = 0; j < NW; ++j) v.w[j] = 0;
    if (wib == 0) {
      if (gr >= 0) v = row_load<NW>(S + (size_t)gr * RD + pcol, lane, RD - pcol);
#pragma unroll
      for (int j = 0; j < NW; ++j) halo_top[lane * NW + j] = v.w[j];
    }
    if (owns_last) {
      const int gb = b0 + nb;
      RowBits<NW> vb;
#pragma unroll
      for (int j = 0; j < NW; ++j) vb.w[j] = 0;
      if (gb < H) vb = row_load<NW>(S + (size_t)gb * RD + pcol, lane, RD - pcol);
#pragma unroll
      for (int j = 0; j < NW; ++j) halo_bot[lane * NW + j] = vb.w[j];
    }
  }
  // Column halos (frames wider than one panel): the strong bits just left / right of the panel, for this wave's
  // rows and the row above / below them -- bit k of the mask = row w0 - 1 + k.  Like the row halos they belong to
  // other workgroups and are as of the start of this launch.
  u64 lmask = 0, rmask = 0;
  if (PANELS && n > 0) {
    const int hr = b0 + w0 - 1 + lane;  // lanes 0 .. n+1 fetch one row each
    const bool rok = lane < n + 2 && hr >= 0 && hr < H;
    const u32 lv = (rok && pn > 0) ? S[(size_t)hr * RD + pcol - 1] : 0u;
    const u32 rv = (rok && pn + 1 < NP) ? S[(size_t)hr * RD + pcol + ROWW] : 0u;
    lmask = uniform64(__ballot((lv >> 31) != 0));
    rmask = uniform64(__ballot((rv & 1u) != 0));
  }
  if (threadIdx.x < 24) bchg[threadIdx.x] = 0;
  __syncthreads();
  const u32 *up_src = wib == 0 ? halo_top : edge + (2 * (wib - 1) + 1) * ROWW;  // row above my first row
  const u32 *dn_src = owns_last ? halo_bot : edge + (2 * (wib + 1)) * ROWW;      // row below my last row

  // Row worklist per wave, lowest dirty row first: a downward sweep that steps back up whenever a
  // row's new strong bits reach candidates of the row above.  Work is proportional to the rows that
  // change.  Waves exchange their boundary rows through LDS between rounds.
  u64 changed = 0;
  u32 colchg = 0;  // bit 0: first column of the panel changed, bit 1: last column
  // First launch, full wave tile: instead of visiting every row once to find out that most have nothing to do (a
  // worklist step costs ~55 instructions even then, more than half of them scalar), the rows that can change at all
  // are found first, all at once: a row is active iff one of its open candidates has a strong 8-neighbour -- in the
  // rows above / below as they are now, or in the row itself.  32 independent tests with compile-time row registers
  // (no s_set_gpr_idx, no dependency between them); every other row is only visited if a neighbour changes later.
  // (Two unrolled sequential sweeps with compile-time registers were tried instead: 63 inlined row updates are 76 KB of
  // code, the instruction cache misses made the hysteresis 1.9x slower.)
  if (NW == 1 && !LATE && n == TR) {
    u64 act = 0;
    auto test_row = [&](auto self, auto rc) {
      constexpr int r = decltype(rc)::value;
      RowBits<NW> nbr;
      const u32 upv = r == 0 ? up_src[lane] : sr[0][r > 0 ? r - 1 : 0];
      const u32 dnv = r == TR - 1 ? dn_src[lane] : sr[0][r < TR - 1 ? r + 1 : 0];
      const u32 sv = sr[0][r], cv = cr[0][r];
      nbr.w[0] = upv | dnv | sv;
      RowBits<NW> d = row_dilate<NW>(nbr);
      if (PANELS) {
        if (((lmask >> r) & 7ull) != 0 && lane == 0) d.w[0] |= 1u;
        if (((rmask >> r) & 7ull) != 0 && lane == 63) d.w[NW - 1] |= 0x80000000u;
      }
      if (__ballot((cv & ~sv & d.w[0]) != 0) != 0) act |= 1ull << r;
      if constexpr (r + 1 < TR) self(self, std::integral_constant<int, r + 1>{});
    };
    test_row(test_row, std::integral_constant<int, 0>{});
    dirty = uniform64(act);
    unfilled = dirty;  // (only) the active rows may still need their first in-row fill: in every other row no open candidate touches a strong bit of the row
  }
  // (HYST_ROUND_CAP, canny_params.h: a budget; a tile that uses it up says so below and goes on in the next launch)
  int round;
  for (round = 0; round < HYST_ROUND_CAP; ++round) {
    u64 round_changed = 0;
    while (dirty) {
      const int r = __builtin_ctzll(dirty);
      dirty &= dirty - 1;
      RowBits<NW> up, dn, s, c;
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        // (index wrapped instead of clamped -- TR is a power of two -- the wrapped row is never the one used)
        up.w[j] = r == 0 ? up_src[lane * NW + j] : sr[j][(r - 1) & (TR - 1)];
        dn.w[j] = r == n - 1 ? dn_src[lane * NW + j] : sr[j][(r + 1) & (TR - 1)];
        s.w[j] = sr[j][r];
        c.w[j] = cr[j][r];
      }
      RowBits<NW> nbr;
#pragma unroll
      for (int j = 0; j < NW; ++j) nbr.w[j] = up.w[j] | dn.w[j];
      RowBits<NW> d = row_dilate<NW>(nbr);
      if (PANELS) {  // a strong pixel in the column next to the panel, rows r-1 .. r+1, touches my first / last column
        if (((lmask >> r) & 7ull) != 0 && lane == 0) d.w[0] |= 1u;
        if (((rmask >> r) & 7ull) != 0 && lane == 63) d.w[NW - 1] |= 0x80000000u;
      }
      RowBits<NW> seed;
      bool grew = false, hs = false, hc = false;
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        seed.w[j] = s.w[j] | (c.w[j] & d.w[j]);
        grew = grew || (seed.w[j] != s.w[j]);
        hs = hs || s.w[j] != 0;
        hc = hc || (c.w[j] & ~s.w[j]) != 0;
      }
      bool todo = __ballot(grew) != 0;
      if ((unfilled >> r) & 1) {
        unfilled &= ~(1ull << r);
        todo = todo || (__ballot(hs) != 0 && __ballot(hc) != 0);
      }
      if (!todo) continue;
      const RowBits<NW> f = row_fill<NW>(c, seed);
      bool ch = false;
#pragma unroll
      for (int j = 0; j < NW; ++j) ch = ch || (f.w[j] != s.w[j]);
      if (__ballot(ch) == 0) continue;
      if (PANELS) {  // did the panel's first / last column change? (lane 0 bit 0, lane 63 bit 31)
        const u32 x0 = f.w[0] ^ s.w[0], x1 = f.w[NW - 1] ^ s.w[NW - 1];
        colchg |= (u32)(__builtin_amdgcn_readlane((int)x0, 0) & 1) | (((u32)__builtin_amdgcn_readlane((int)x1, 63) >> 31) << 1);
      }
#pragma unroll
      for (int j = 0; j < NW; ++j) sr[j][r] = f.w[j];
      if (r == 0) publish(my_first, 0);
      if (r == n - 1) publish(my_last, n - 1);
      round_changed |= 1ull << r;
      // The row below is looked at again in any case.  The row above only if a new bit reaches one of its open
      // candidates: it is at its own fixpoint for everything but this change (in a downward sweep nearly every step
      // used to be followed by a second look at the row above that found nothing).
      dirty |= ((1ull << r) << 1) & all_rows;
      if (r > 0) {
        RowBits<NW> nb;
#pragma unroll
        for (int j = 0; j < NW; ++j) nb.w[j] = f.w[j] & ~s.w[j];
        const RowBits<NW> reach = row_dilate<NW>(nb);
        bool hit = false;
#pragma unroll
        for (int j = 0; j < NW; ++j) hit = hit || (reach.w[j] & cr[j][r - 1] & ~sr[j][r - 1]) != 0;
        if (__ballot(hit) != 0) dirty |= (1ull << r) >> 1;
      }
    }
    changed |= round_changed;
    if (lane == 0) bchg[wib] = (n > 0 && (round_changed & 1ull) ? 1u : 0u) | (n > 0 && ((round_changed >> (n - 1)) & 1ull) ? 2u : 0u);
    __syncthreads();
    if (n > 0) {
      if (wib > 0 && (bchg[wib - 1] & 2u)) dirty |= 1ull;
      if (!owns_last && wib + 1 < WAVES && (bchg[wib + 1] & 1u)) dirty |= 1ull << (n - 1);
    }
    dirty = uniform64(dirty);
    // workgroup-wide "any wave has work": OR through an LDS word per round parity
    if (lane == 0 && dirty != 0) atomicOr(&bchg[18 + (round & 1)], 1u);
    __syncthreads();
    const bool more = __builtin_amdgcn_readfirstlane(bchg[18 + (round & 1)]) != 0;
    if (threadIdx.x == 0) bchg[18 + ((round + 1) & 1)] = 0;
    if (!more) break;
  }
  // Out of rounds with rows still open: the tile is not at its fixpoint, and nobody else may know -- its boundary rows and
  // columns need not have changed.  It flags the launch and leaves ITSELF the reason that reopens all its rows (`side`) for
  // the next launch, as a neighbour would (below); what it reached so far goes to the plane and the map as usual.
  const bool capped = round == HYST_ROUND_CAP;  // uniform for the workgroup: every wave saw the same `more`

  // Rows that changed go back to the plane, and the 0/255 map is written (removeCandidates + output copy,
  // cannyEdgeD.cu:379-395: strong bits -> 255, rest 0; 16 px per lane per store).  When the output already shows
  // the planes as they were in memory -- k_nms wrote the strong pixels (p.prov), or an earlier launch left it so --
  // only the 16-pixel groups whose bits changed are rewritten: the old dword of a row is read back (one row ahead)
  // and compared with the new one.  A changed row typically has two or three such groups out of 120, so they are not
  // expanded row by row (a few active lanes per instruction) but collected in a wave-private LDS queue -- one dword
  // per group: its 16 bits, row and position -- and expanded 64 at a time, a group per lane.  Dense content is the exception
  // (iid noise: a changed row has 87 changed groups at the median, profiles/r16_dense_rows/groups_per_row.txt): a row with
  // HYST_ROW_FULL changed groups or more (canny_params.h) skips the queue and is written whole, as launch 0 of a run without a
  // provisional map writes every row (expand_rows).
  {
    const bool patch = p.out && (LATE || p.prov);
    const bool a16 = (((uintptr_t)p.out | p.out_pitch | p.out_frame_stride) & 15u) == 0;
    uint8_t *obase = p.out ? p.out + (size_t)frame * p.out_frame_stride : nullptr;
    u32 *Sw = S + (size_t)(b0 + w0) * RD;  // the wave's first row (uniform); this lane's dword is at pcol + lane
    const u32 s_lane = (u32)(pcol + lane);
    uint8_t *out0 = obase + (size_t)(b0 + w0) * p.out_pitch;  // the wave's first row in the map (only used with p.out)
    // 16 pixels whose bits are `b`, starting at column c0 of row `row` of this frame
    auto put16 = [&](u32 b, int row, int c0) {
      if (c0 >= p.W) return;
      u32 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = nibble_to_bytes((b >> (4 * k)) & 0xFu);
      uint8_t *dst = obase + (size_t)row * p.out_pitch + c0;
      if (c0 + 15 < p.W) {
        if (a16) {
          // (the pointer goes through an empty asm: seeing two branches that store the same bytes, the optimizer otherwise
          //  merges them into the four dword stores -- twice the store instructions of the full-map launch)
          uint8_t *d16 = dst;
          asm volatile("" : "+v"(d16));
          *reinterpret_cast<uint4 *>(d16) = make_uint4(v[0], v[1], v[2], v[3]);
        } else
#pragma unroll
          for (int k = 0; k < 4; ++k) reinterpret_cast<u32 *>(dst)[k] = v[k];
      } else {
#pragma nounroll  // (unrolled, the 16 exec masks of this ragged last group cost the kernel an SGPR spill, i.e. a VGPR: 81 instead of 80)
        for (int k = 0; k < 16 && c0 + k < p.W; ++k) dst[k] = ((b >> k) & 1u) ? (uint8_t)255 : (uint8_t)0;
      }
    };
    u32 *xq = xqueue + wib * XQ_CAP;  // ring of changed groups: bits | row (6 bits) << 16 | group-of-the-panel-row << 22
    int xhead = 0, xcount = 0;
    auto xflush = [&](int nent) {
      wave_lds_sync();
      const u32 ent = xq[(xhead + lane) & (XQ_CAP - 1)];
      if (lane < nent) put16(ent & 0xFFFFu, b0 + w0 + (int)((ent >> 16) & 63u), pcol * 32 + (int)(ent >> 22) * 16);
      xhead = (xhead + nent) & (XQ_CAP - 1);
      xcount -= nent;
    };
    u64 whole = 0;  // rows that go to the map whole, after the groups of the others: all of them, or the changed rows with HYST_ROW_FULL changed groups or more
    if (p.out && !patch) {
      // first launch on planes the output does not show yet: every row of the tile, whole rows, two passes of 64 groups
      for (u64 m = changed; m != 0; m &= m - 1) {
        const int r = __builtin_ctzll(m);
        (Sw + (size_t)r * RD)[s_lane] = sr[0][r];
      }
      whole = all_rows;
    } else {
      u64 m = changed;
      typedef u32 Old16 __attribute__((ext_vector_type(16)));
      for (;;) {
        if (xcount >= 64 || (m == 0 && xcount > 0)) {  // the one place where groups are expanded
          xflush(min(xcount, 64));
          continue;
        }
        if (m == 0) break;
        // What the plane (and with it the output) showed before this launch, for the next up to 16 changed rows: all
        // requests at once, one wait.  (Read back one row ahead inside the loop, each changed row waited for its own
        // load and -- the load being conditional -- for the stores before it as well.)
        Old16 oldv;
        if (patch) {
          u64 mb = m;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            u32 v = 0;
            if (mb) {
              v = (Sw + (size_t)__builtin_ctzll(mb) * RD)[s_lane];
              mb &= mb - 1;
            }
            oldv[j] = v;
          }
        }
        for (int j = 0; j < 16 && m != 0 && xcount < 64; ++j) {
          const int r = __builtin_ctzll(m);
          m &= m - 1;
          const u32 rowv = sr[0][r];
          (Sw + (size_t)r * RD)[s_lane] = rowv;
          if (!patch) continue;  // no output at all (hc_hysteresis_device on planes only)
          const u32 dv = oldv[j] ^ rowv;
          const bool clo = (dv & 0xFFFFu) != 0, chi = (dv >> 16) != 0;
          const u64 mlo = __ballot(clo), mhi = __ballot(chi);
          if ((mlo | mhi) == 0) continue;
          u32 nlo, nhi;
          asm("s_bcnt1_i32_b64 %0, %1" : "=s"(nlo) : "s"(mlo) : "scc");
          asm("s_bcnt1_i32_b64 %0, %1" : "=s"(nhi) : "s"(mhi) : "scc");
          if (nlo + nhi >= (u32)HYST_ROW_FULL) {  // (wave-uniform) most of the row changed: the whole row below, nothing queued
            whole |= 1ull << r;
            continue;
          }
          const u32 base = (u32)(xhead + xcount), tag = (u32)r << 16;
          if (clo) xq[(base + mbcnt64(mlo)) & (XQ_CAP - 1)] = (rowv & 0xFFFFu) | tag | ((u32)(2 * lane) << 22);
          if (chi) xq[(base + nlo + mbcnt64(mhi)) & (XQ_CAP - 1)] = (rowv >> 16) | tag | ((u32)(2 * lane + 1) << 22);
          xcount += (int)(nlo + nhi);
        }
      }
    }
    // (patching, a group that did not change gets the bytes it holds: the map shows the plane, and the row belongs to this wave alone)
    if (whole != 0) {
      // (the lane index through an empty asm: what expand_rows derives from it -- half-word, column, byte offsets -- is
      //  otherwise computed ahead of the tile loop and held in registers through it: 82 VGPRs in two instances)
      int xlane = lane;
      asm volatile("" : "+v"(xlane));
      expand_rows<ROWW>(sr[0], whole, out0, p.out_pitch, pcol, p.W, a16, xlane);
    }
  }
  const bool first_changed = n > 0 && w0 == 0 && (changed & 1ull);
  const bool last_changed = owns_last && ((changed >> (n - 1)) & 1ull);
  if (lane == 0 && (first_changed || last_changed || colchg)) atomicOr(&bchg[16], (first_changed ? 1u : 0u) | (last_changed ? 2u : 0u) | (colchg << 2));
  __syncthreads();
  if (MODE == HYST_PER_TILE) {
    // the tiles that look at what changed get their reason (no list: every launch starts a workgroup per tile, and a tile
    // without a reason leaves after one load).  One lane per neighbour, as below; lane 8: the tile itself, out of rounds.
    if (wib == 0) {
      const u32 vis = bchg[16] | (capped ? 16u : 0u);  // bit 4: out of rounds (lane 8 below)
      if (vis != 0) {
        if (lane == 0) atomicOr(&p.flags[p.iter], 1u);
        u32 *reason = p.wl_reason + (size_t)((p.iter + 1) & 1) * p.wl_stride;
        const int k = lane;
        const int t = k < 3 ? bt + 1 : k < 6 ? bt - 1 : bt;
        const int q = k < 6 ? pn + (k % 3) - 1 : (k == 6 ? pn - 1 : k == 7 ? pn + 1 : pn);
        const u32 need = k < 3 ? 2u : k < 6 ? 1u : k == 6 ? 4u : k == 7 ? 8u : 16u;
        const u32 why = k < 3 ? 1u : k < 6 ? 2u : 4u;
        if (k < 9 && (vis & need) != 0 && t >= 0 && t < p.nrtiles && q >= 0 && q < NP) atomicOr(&reason[frame * ntile + t * NP + q], why);
      }
    }
  } else if (wib == 0) {
    // The neighbours that look at what changed go on the next launch's worklist -- once each: the first reason to arrive
    // appends the tile, later ones only add their bit.  One lane per neighbour, so that the atomics' round trips overlap.
    const u32 vis = bchg[16] | (capped ? 16u : 0u);  // bit 4: out of rounds (lane 8 below)
    if (vis != 0) {
      if (lane == 0) atomicOr(&p.flags[p.iter], 1u);
      const int nxt = (p.iter + 1) & 1;
      u32 *reason = p.wl_reason + (size_t)nxt * p.wl_stride, *list = p.wl_list + (size_t)nxt * p.wl_stride;
      // lanes 0-2: the tiles below (my last row changed: their `top`), 3-5: above (my first row: their `bot`), 6 / 7: the
      // panel left / right (my first / last column: their `side`), 8: this tile itself when it ran out of rounds (its own
      // `side`: every row open again)
      const int k = lane;
      const int t = k < 3 ? bt + 1 : k < 6 ? bt - 1 : bt;
      const int q = k < 6 ? pn + (k % 3) - 1 : (k == 6 ? pn - 1 : k == 7 ? pn + 1 : pn);
      const u32 need = k < 3 ? 2u : k < 6 ? 1u : k == 6 ? 4u : k == 7 ? 8u : 16u;
      const u32 why = k < 3 ? 1u : k < 6 ? 2u : 4u;
      if (k < 9 && (vis & need) != 0 && t >= 0 && t < p.nrtiles && q >= 0 && q < NP) {
        const u32 g = (u32)(frame * ntile + t * NP + q);
        if (atomicOr(&reason[g], why) == 0) list[atomicAdd(&p.wl_count[p.iter + 1], 1u)] = g;
      }
    }
  }
  if (lane == 0 && p.stats && n > 0) {  // diagnostics (opt-in): changed rows summed / max over wave tiles, active wave tiles
    const u32 nch = (u32)__builtin_popcountll(changed);
    atomicAdd(&p.stats[0], nch);
    atomicMax(&p.stats[1], nch);
    atomicAdd(&p.stats[2], 1u);
  }
}

// HYST_PER_TILE / HYST_PER_TILE_TO_LIST (frames of one column panel, up to 2048 columns; dense wide frames -- their launches 0 to 2): a workgroup per
// tile; a tile whose neighbours left it no reason exits after one load.
// HYST_LIST_FIRST / HYST_LIST_LATE (wider frames): launch 0 as above; launch k > 0 takes its tiles from the worklist its predecessor wrote --
// the tiles whose neighbours changed a boundary row / column -- with a grid that is a fraction of the tile count
// (launch_hyst), one list entry per workgroup.  With panels a tile has eight neighbours, the flag test of HYST_PER_TILE is nine
// dependent byte loads, and the late launches that follow the few long edges of a frame through its tiles each started
// 17 k workgroups to find 1-2 % of them with work: on 4K and 8K streams most of the hysteresis chain's time, which is
// what their step follows (4K 100 -> 108 k frames/s, 8K x 3 channels 7.4 -> 8.3 k, 8K grey 15.8 -> 19.7 k).  At 1080p
// the flags are better: 388 k against 378 k frames/s -- there the step follows the front kernel, and a hysteresis that
// is spread thinly over it costs it less than the same work done in two thirds of the time (1.64 against 2.27 ms).
// No loop over list entries: around the tile code it costs registers (85-91 VGPRs; 148 and a stack as a real function),
// and the tile code must stay at 80 -- two hysteresis waves per 160-register hole a retiring front wave leaves.  Entries
// beyond the grid (dense or adversarial content: more than the grid's share of the tiles still active) are handed on to
// the next launch's list instead.
template <int NW, int TR, int WAVES, bool PANELS, int MODE>
__global__ __launch_bounds__(WAVES * 64) void k_hyst(const HystParams p)
{
  if ((MODE == HYST_PER_TILE || MODE == HYST_PER_TILE_TO_LIST) && p.iter > 0 && p.flags[p.iter - 1] == 0) return;  // previous launch changed no tile boundary: fixpoint reached
  // latency-bound kernel (a few waves walking dependent row steps): when it shares a SIMD with the next
  // run's front waves (pipelined mode) it should win the instruction arbitration
  __builtin_amdgcn_s_setprio(3);
  if constexpr (MODE != HYST_LIST_LATE) {
    hyst_tile<NW, TR, WAVES, PANELS, MODE>(p, (int)blockIdx.x, false, false, false);
  } else {
    const u32 cnt = p.wl_count[p.iter];  // 0: the previous launch changed no tile boundary, the fixpoint is reached
    if (blockIdx.x >= cnt) return;
    const u32 *list = p.wl_list + (size_t)(p.iter & 1) * p.wl_stride;
    u32 *reason = p.wl_reason + (size_t)(p.iter & 1) * p.wl_stride;
    if (cnt > gridDim.x && threadIdx.x == 0 && blockIdx.x + gridDim.x < cnt) {
      const int nxt = (p.iter + 1) & 1;
      u32 *reason_n = p.wl_reason + (size_t)nxt * p.wl_stride, *list_n = p.wl_list + (size_t)nxt * p.wl_stride;
      for (u32 j = blockIdx.x + gridDim.x; j < cnt; j += gridDim.x) {
        const u32 g2 = list[j], w2 = reason[g2];
        reason[g2] = 0;
        if (atomicOr(&reason_n[g2], w2) == 0) list_n[atomicAdd(&p.wl_count[p.iter + 1], 1u)] = g2;
      }
      atomicOr(&p.flags[p.iter], 1u);  // work is left for another launch
    }
    const u32 g = (u32)__builtin_amdgcn_readfirstlane((int)list[blockIdx.x]);
    const u32 why = (u32)__builtin_amdgcn_readfirstlane((int)reason[g]);
    __syncthreads();  // everyone has the reason before it is cleared for launch k + 2
    if (threadIdx.x == 0) reason[g] = 0;
    hyst_tile<NW, TR, WAVES, PANELS, HYST_LIST_LATE>(p, (int)g, (why & 1u) != 0, (why & 2u) != 0, (why & 4u) != 0);
  }
}

// ---- one launch for the whole hysteresis of a small run -------------------------------------------------------------
// A run of a few frames (the reference's one-frame-per-call pattern and the small pipelined batches) has at most a few
// dozen workgroup tiles, all resident at once, and its K dependent launches are K host calls and K trips through the
// command processor for kernels that mostly find nothing to do.  k_hyst_loop runs the same rounds -- hyst_tile in its
// workgroup-per-tile form, round `it` exactly what launch `it` would have been -- inside ONE launch, separated by a
// device-wide barrier: every workgroup releases its stores (the XCDs' L2s are not coherent with each other: agent-scope
// release = write-back, acquire = invalidate), arrives at a counter in device memory, waits for the others, acquires.
// The flag word of a round tells all workgroups alike whether another round is needed.
// Every wait is bounded: a workgroup that does not see the others arrive within ~4 ms (they are not resident -- another
// process fills the device) raises the abort word, marks the run as not converged and leaves; so do the others when
// they see it.  The host then continues the run with ordinary launches (finish_slot), as after any run whose queued
// launches were too few.  The grid never waits for a workgroup that cannot come.
static __device__ __forceinline__ bool grid_barrier(u32 *bar, u32 target)
{
  __shared__ u32 ok;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(&bar[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    u32 good = 1;
    for (u32 spin = 0;; ++spin) {
      if (__hip_atomic_load(&bar[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) break;
      if (spin > 4000u || __hip_atomic_load(&bar[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
        __hip_atomic_store(&bar[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        good = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
    ok = good;
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return ok != 0;
}

template <int TR, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_hyst_loop(const HystParams p0, int rounds, u32 *bar)
{
  __builtin_amdgcn_s_setprio(3);
  HystParams p = p0;
  for (int it = 0; it < rounds; ++it) {
    p.iter = it;
    hyst_tile<1, TR, WAVES, false, HYST_PER_TILE>(p, (int)blockIdx.x, false, false, false);
    if (it + 1 == rounds) return;  // (the host reads this round's flag: set = not converged, finish_slot continues)
    if (!grid_barrier(bar, gridDim.x * (u32)(it + 1))) {
      if (threadIdx.x == 0) atomicOr(&p.flags[rounds - 1], 1u);
      return;
    }
    if (__hip_atomic_load(&p.flags[it], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;  // no tile boundary changed: the fixpoint (the same answer in every workgroup)
  }
}

// Calls f(TR, WAVES) -- two std::integral_constant<int> -- for the entry (tile_rows, waves) of HYST_SHAPES: the table is
// walked at compile time, so f is instantiated once per shape.  False: no such shape.
template <class F, size_t... I>
static bool for_hyst_shape(int tile_rows, int waves, F &&f, std::index_sequence<I...>)
{
  return ((tile_rows == HYST_SHAPES[I].tile_rows && waves == HYST_SHAPES[I].waves
           && (f(std::integral_constant<int, HYST_SHAPES[I].tile_rows>{}, std::integral_constant<int, HYST_SHAPES[I].waves>{}), true)) || ...);
}
template <class F>
static bool for_hyst_shape(int tile_rows, int waves, F &&f) { return for_hyst_shape(tile_rows, waves, f, std::make_index_sequence<N_HYST_SHAPES>{}); }

// rounds <= MAX launches of the workgroup-per-tile form in one launch; the caller guarantees one column panel, at most
// HYST_LOOP_MAX_TILES tiles (resident together, with room for the loops of the other runs in flight) and bar[0..1] == 0
hipError_t launch_hyst_loop(const HystParams &p, int rounds, u32 *bar, hipStream_t s)
{
  const size_t tiles = (size_t)p.nframes * p.nrtiles;
  if (p.npanels != 1 || p.RD != 64 || tiles == 0 || tiles > (size_t)HYST_LOOP_MAX_TILES || rounds < 1 || !bar || !p.wl_reason || p.wl_stride < tiles) return hipErrorInvalidValue;
  bool launched = false;
  for_hyst_shape(p.tile_rows, p.waves, [&](auto tr, auto waves) {
    if constexpr (hyst_shape_loops(tr, waves)) {
      hipLaunchKernelGGL((k_hyst_loop<tr, waves>), dim3((unsigned)tiles), dim3(64 * waves), 0, s, p, rounds, bar);
      launched = true;
    }
  });
  return launched ? hipGetLastError() : hipErrorInvalidValue;
}

// one launch of one shape: the kernel for (PANELS, mode); a lane always holds one dword per row (NW = 1, see hyst_tile)
template <int TR, int WAVES, bool PANELS>
static void launch_hyst_shape(const HystParams &p, HystMode mode, dim3 grid, hipStream_t s)
{
  const dim3 block(64 * WAVES);
  switch (mode) {
  case HYST_PER_TILE: hipLaunchKernelGGL((k_hyst<1, TR, WAVES, PANELS, HYST_PER_TILE>), grid, block, 0, s, p); break;
  case HYST_LIST_FIRST: hipLaunchKernelGGL((k_hyst<1, TR, WAVES, PANELS, HYST_LIST_FIRST>), grid, block, 0, s, p); break;
  case HYST_LIST_LATE: hipLaunchKernelGGL((k_hyst<1, TR, WAVES, PANELS, HYST_LIST_LATE>), grid, block, 0, s, p); break;
  case HYST_PER_TILE_TO_LIST: hipLaunchKernelGGL((k_hyst<1, TR, WAVES, PANELS, HYST_PER_TILE_TO_LIST>), grid, block, 0, s, p); break;
  }
}

hipError_t launch_hyst(const HystParams &p, hipStream_t s)
{
  if (p.RD > 256) return hipErrorInvalidValue;
  if (p.npanels != (p.RD + 63) / 64 || p.RD % 64) return hipErrorInvalidValue;
  const size_t tiles = (size_t)p.nframes * p.nrtiles * p.npanels;
  const bool wide = p.npanels > 1;
  const HystMode mode = hyst_mode(p.lists, p.iter);
  if (tiles > 0x7FFFFFFFull || !p.wl_reason || p.wl_stride < tiles) return hipErrorInvalidValue;
  if ((wide || p.lists != 0) && (!p.wl_count || !p.wl_list)) return hipErrorInvalidValue;
  // a workgroup per tile -- except the later launches of the worklist scheme: a workgroup per list entry.  Grid: the
  // caller's (p.late_grid, from the last run's list lengths), or a schedule that shrinks to an eighth of the tiles (at
  // least 2048 workgroups): on camera-like frames a third of the tiles are listed for launch 1, 1-2 % from launch 5 on;
  // entries beyond the grid wait for the next launch (k_hyst).
  size_t wgs = tiles;
  if (mode == HYST_LIST_LATE) {
    wgs = std::min(tiles, std::max<size_t>(2048, tiles >> std::min(std::max(p.iter - 2, 0), 3)));
    if (p.late_grid > 0) wgs = std::min(tiles, (size_t)p.late_grid);
  }
  const dim3 grid((unsigned)wgs);
  const bool known = for_hyst_shape(p.tile_rows, p.waves, [&](auto tr, auto waves) {
    if (wide) launch_hyst_shape<tr, waves, true>(p, mode, grid, s);
    else launch_hyst_shape<tr, waves, false>(p, mode, grid, s);
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace hc
