// morph.hip -- k_morph8: one K x K maximum filter launch of hc_morphology_device (cv::dilate; on complemented bytes cv::erode).
//
//   u8 frames (1 or 3 interleaved channels) -> u8 frames with the same interleave.  The element is K half-widths: row j covers
//   the columns -span[j] .. +span[j] around the anchor, -1 an empty row; out(y, x) = max over j, dx of src(y + j - K/2, x + dx).
// Layout as k_gauss8: a wave owns a 248-column strip, lane l the 4 pixels at strip * 248 - 4 + 4 l, lanes 0 and 63 are halo.  A
// work item is (frame, strip, BLUR_CHUNK_ROWS rows) with a warm-up of K - 1 rows; rows are requested K steps ahead.  No LDS, no
// atomics, registers only; every ring slot is a compile-time index.
// Arithmetic: packed u16 maxima on pixel pairs (v_pk_max_u16).  The horizontal maxima nest: m_0 = the row, m_a = max(m_(a-1), the
// row shifted by +a and by -a), so one pass over the pair window gives every half-width.  A source row serves K output rows, each
// time as another element row, so the ring keeps of each of the last K rows one horizontal maximum per DISTINCT half-width of the
// element (NLEV "levels", wave-uniform; a RECT has one and the filter is separable); an output row takes of ring row j the level
// of element row j, chosen wave-uniformly.  Ring entries are pixel pairs where that fits the register budget (WIDE), else the 4
// pixels packed as bytes, unpacked again for the vertical maximum.
// Erode is the same kernel on complemented bytes (x ^ 0xff after the load and before the store, wave-uniform).
// Border: positions outside the frame never take part.  Lanes and bytes outside the row hold 0, the identity of the maximum (also
// after the complement: only bytes inside the row are complemented); rows above and below the frame are not loaded and enter the
// ring as zeros, wave-uniformly.  No border index is mapped.  A window wholly outside gives 0: dilate 0, erode 255.
// GRADIENT needs both extremes: a second launch computes the erosion and stores (what the output holds) - erosion, saturated (0
// where the window holds no pixel of the frame), the first having left the dilation there (two rings in one pass would not fit 128 registers at K = 7 with 3 channels).
// Memory: as k_gauss8 -- no byte outside [row, row + C W) of an input or output row is read or written, at any alignment: dword
// loads and stores only for whole 4-pixel groups of 4-aligned rows (in_aligned / out_aligned), bytes otherwise.  Rows are addressed
// with 32-bit offsets (H * pitch < 2^32 on both sides: plan_morphology).  The row source and the interleaving store repeat those
// of blur.hip (DESIGN.md 3.7j says why they are not shared).
#include "sep_deriv.h"

namespace hc {

namespace {

using namespace sep;

static __device__ __forceinline__ u32 pk_max(u32 a, u32 b) { return R(__builtin_elementwise_max(U(a), U(b))); }
// wave-uniform cond ? a : b as one v_cndmask the compiler cannot see through: chains of plain selects over ring entries it turned
// into dynamic indexing, and the ring went to scratch memory (3 and 4 levels)
static __device__ __forceinline__ u32 uni_sel(bool cond, u32 a, u32 b) { return lane_sel(uniform64(cond ? ~0ull : 0ull), a, b); }
// the 4 pixels of two pairs as bytes
static __device__ __forceinline__ u32 pack_pairs(u32 lo, u32 hi) { return __builtin_amdgcn_perm(hi, lo, 0x06040200u); }

template <int K, int NC, int NLEV>
__global__ __launch_bounds__(256) void k_morph8(const MorphParams p)
{
  constexpr int RAD = K / 2;
  constexpr bool WIDE = NLEV * K * NC * 2 <= 48;  // ring entries as pixel pairs (2 registers), else as bytes (1)
  constexpr int RW = WIDE ? 2 : 1;
  constexpr int NCAND = RAD - NLEV + 2;           // level l is one of the half-widths l .. l + NCAND - 1 (distinct, ascending)
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const int item = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + wib);
  if (item >= p.total_items) return;
  const int chunk = item % p.nchunks;
  const int strip = (item / p.nchunks) % p.nstrips;
  const int frame = item / (p.nchunks * p.nstrips);
  const int W = p.W, H = p.H;
  const int r0 = chunk * BLUR_CHUNK_ROWS, rend = min(r0 + BLUR_CHUNK_ROWS, H);
  const int c0 = strip * BLUR_STRIP_W - STRIP_HALO + lane * PX_PER_LANE;
  const int vlast = min(rend - 1 + RAD, H - 1);  // last source row this item loads

  // the element, wave-uniform
  int lev[NLEV], rlev[K];
#pragma unroll
  for (int l = 0; l < NLEV; ++l) lev[l] = __builtin_amdgcn_readfirstlane((int)p.level[l]);
#pragma unroll
  for (int j = 0; j < K; ++j) rlev[j] = __builtin_amdgcn_readfirstlane((int)p.row_level[j]);
  const u32 cm = p.complement ? 0xFFFFFFFFu : 0u;

  // columns: c0 is a multiple of 4, so a lane's 4 columns lie inside the row (`inside`), partly (the row's last lane) or not at all
  const int n_in = c0 < 0 ? 0 : min(4, max(W - c0, 0));  // the lane's columns inside the row
  const int n_el = NC * n_in;                            // ... and their bytes
  const bool inside = n_in == 4;
  const bool fast_ld = inside && p.in_aligned;
  const bool byte_ld = n_in > 0 && !fast_ld;
  const uint8_t *fbase = p.in + (size_t)frame * p.in_frame_stride + (size_t)NC * (size_t)max(c0, 0);
  const u32 in_pitch = (u32)p.in_pitch;
  struct Raw { u32 d[NC]; };  // the lane's 4 pixels as they lie in memory, complemented where asked: 4 NC interleaved bytes
  u32 xm[NC];                 // the complement of the bytes inside the row only: the others stay 0
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int nb = min(4, max(n_el - 4 * i, 0));
    xm[i] = cm & (nb == 4 ? 0xFFFFFFFFu : (1u << (8 * nb)) - 1u);
  }
  auto load_row = [&](int vrow) -> Raw {
    Raw r;
#pragma unroll
    for (int i = 0; i < NC; ++i) r.d[i] = 0;
    if (vrow < 0 || vrow > vlast) return r;  // wave-uniform: rows outside the frame (or this item's reach) are not loaded
    const uint8_t *rp = fbase + (u32)vrow * in_pitch;
    if (fast_ld) {
      const u32 *q = reinterpret_cast<const u32 *>(rp);
#pragma unroll
      for (int i = 0; i < NC; ++i) r.d[i] = q[i];
    } else if (byte_ld) {
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        u32 v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (4 * i + b < n_el) v |= (u32)rp[4 * i + b] << (8 * b);
        r.d[i] = v;
      }
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) r.d[i] ^= xm[i];
    return r;
  };
  // channel ch of the 4 pixels as one dword: of 12 interleaved bytes the channel's (ch, ch + 3, ch + 6, ch + 9)
  auto channel_of = [](const u32 (&d)[NC], int ch) -> u32 {
    if constexpr (NC == 1) return d[0];
    else {
      const u32 selA = ch == 0 ? 0x0c060300u : ch == 1 ? 0x0c070401u : 0x0c0c0502u;
      const u32 selB = ch == 0 ? 0x05020100u : ch == 1 ? 0x06020100u : 0x07040100u;
      return __builtin_amdgcn_perm(d[2], __builtin_amdgcn_perm(d[1], d[0], selA), selB);
    }
  };

  // per channel: of the last K source rows the horizontal maximum of each level [ring][level][pair, or the 4 bytes]
  u32 HR[NC][K][NLEV][RW];
#pragma unroll
  for (int ch = 0; ch < NC; ++ch)
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
      for (int l = 0; l < NLEV; ++l)
#pragma unroll
        for (int w = 0; w < RW; ++w) HR[ch][a][l][w] = 0;

  const bool st_lane = lane >= 1 && lane <= 62 && c0 < W;
  const bool st_fast = c0 + 3 < W && p.out_aligned;
  uint8_t *const obase = p.out + (size_t)frame * p.out_frame_stride + (size_t)NC * (size_t)max(c0, 0);
  const u32 out_pitch = (u32)p.out_pitch;
  const bool subtract = p.subtract != 0;

  // one step: source row k arrives -> output row g = k - RAD
  auto step = [&](auto uc, int k, const Raw &raw) {
    constexpr int u = decltype(uc)::value;
    const int g = k - RAD;
    const bool emit = g >= r0 && g < rend;  // wave-uniform
    const bool live = k >= 0 && k <= vlast;  // wave-uniform: the row lies inside the frame
    u32 B[NC];                               // per channel: the 4 output pixels
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
      if (live) {
        const PairWindow P = sep_window(channel_of(raw.d, ch));
        u32 m[RAD + 1][2];  // the nested maxima of both pairs
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int c = 4 + 2 * h;
          m[0][h] = P.p[c];
#pragma unroll
          for (int a = 1; a <= RAD; ++a) m[a][h] = pk_max(m[a - 1][h], pk_max(P.p[c - a], P.p[c + a]));
        }
#pragma unroll
        for (int l = 0; l < NLEV; ++l) {
          u32 s0 = m[l][0], s1 = m[l][1];
#pragma unroll
          for (int a = l + 1; a < l + NCAND; ++a) {
            s0 = uni_sel(lev[l] >= a, m[a][0], s0);
            s1 = uni_sel(lev[l] >= a, m[a][1], s1);
          }
          if constexpr (WIDE) { HR[ch][u][l][0] = s0; HR[ch][u][l][1] = s1; }
          else HR[ch][u][l][0] = pack_pairs(s0, s1);
        }
      } else {
#pragma unroll
        for (int l = 0; l < NLEV; ++l)
#pragma unroll
          for (int w = 0; w < RW; ++w) HR[ch][u][l][w] = 0;
      }
      if (emit) {  // vertical maximum over source rows k - K + 1 .. k: element row j takes ring slot (u + 1 + j) % K
        u32 a0 = 0, a1 = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const int slot = (u + 1 + j) % K;
          if (rlev[j] < 0) continue;  // an empty row (wave-uniform)
          u32 v[RW];
#pragma unroll
          for (int w = 0; w < RW; ++w) {
            v[w] = HR[ch][slot][0][w];
#pragma unroll
            for (int l = 1; l < NLEV; ++l) v[w] = uni_sel(rlev[j] >= l, HR[ch][slot][l][w], v[w]);
          }
          if constexpr (WIDE) { a0 = pk_max(a0, v[0]); a1 = pk_max(a1, v[1]); }
          else { a0 = pk_max(a0, unpack_lo(v[0])); a1 = pk_max(a1, unpack_hi(v[0])); }
        }
        B[ch] = pack_pairs(a0, a1);
      }
    }
    if (emit && st_lane) {
      u32 w[NC];
      if constexpr (NC == 1) w[0] = B[0];
      else {  // interleave: byte 3 q + ch
        w[0] = __builtin_amdgcn_perm(B[2], __builtin_amdgcn_perm(B[1], B[0], 0x010c0400u), 0x03040100u);
        w[1] = __builtin_amdgcn_perm(B[2], __builtin_amdgcn_perm(B[1], B[0], 0x06020c05u), 0x03020500u);
        w[2] = __builtin_amdgcn_perm(B[2], __builtin_amdgcn_perm(B[1], B[0], 0x0c07030cu), 0x07020106u);
      }
#pragma unroll
      for (int j = 0; j < NC; ++j) w[j] ^= cm;
      uint8_t *q = obase + (u32)g * out_pitch;
      // a window with no row inside the frame (wave-uniform: a row that is not empty always holds its own column): the dilation
      // is 0 and the erosion 255 there, and the saturated difference 0
      bool window = false;
#pragma unroll
      for (int j = 0; j < K; ++j) window = window || (rlev[j] >= 0 && g + j - RAD >= 0 && g + j - RAD < H);
      if (st_fast) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          // bytewise: where the window holds a pixel no byte of the erosion exceeds the dilation's, so no borrow crosses a byte
          if (subtract) w[j] = window ? reinterpret_cast<const u32 *>(q)[j] - w[j] : 0u;
          reinterpret_cast<u32 *>(q)[j] = w[j];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4 * NC; ++e)
          if (e < n_el) {
            const uint8_t b = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
            q[e] = subtract ? (window ? (uint8_t)(q[e] - b) : (uint8_t)0) : b;
          }
      }
    }
  };

  // source rows r0 - RAD .. rend - 1 + RAD, K steps per loop trip (the ring period); a row is requested K steps before it is used
  const int k0 = r0 - RAD, kend = rend + RAD;
  Raw bn[K];
#pragma unroll
  for (int j = 0; j < K; ++j) bn[j] = load_row(k0 + j);
  auto advance = [&](auto uc, int k) {
    constexpr int j = decltype(uc)::value;
    const Raw b = bn[j];
    bn[j] = load_row(k + K);
    step(uc, k, b);
  };
#pragma nounroll
  for (int k = k0; k < kend; k += K) {
    advance(std::integral_constant<int, 0>{}, k + 0);
    advance(std::integral_constant<int, 1>{}, k + 1);
    advance(std::integral_constant<int, 2>{}, k + 2);
    if constexpr (K > 3) {
      advance(std::integral_constant<int, 3>{}, k + 3);
      advance(std::integral_constant<int, 4>{}, k + 4);
    }
    if constexpr (K > 5) {
      advance(std::integral_constant<int, 5>{}, k + 5);
      advance(std::integral_constant<int, 6>{}, k + 6);
    }
  }
}

template <int K, int NLEV>
void launch_kl(const MorphParams &p, const dim3 grid, const dim3 block, hipStream_t s)
{
  if constexpr (NLEV <= K / 2 + 1) {
    if (p.channels == 3) hipLaunchKernelGGL((k_morph8<K, 3, NLEV>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((k_morph8<K, 1, NLEV>), grid, block, 0, s, p);
  }
}

template <int K>
void launch_k(const MorphParams &p, const dim3 grid, const dim3 block, hipStream_t s)
{
  switch (p.nlevels) {
  case 1: launch_kl<K, 1>(p, grid, block, s); break;
  case 2: launch_kl<K, 2>(p, grid, block, s); break;
  case 3: launch_kl<K, 3>(p, grid, block, s); break;
  default: launch_kl<K, 4>(p, grid, block, s); break;
  }
}

}  // namespace

hipError_t launch_morph8(const MorphParams &p, hipStream_t s)
{
  bool ok = p.W >= 1 && p.H >= 1 && p.nframes >= 1 && (p.channels == 1 || p.channels == 3) && blur_ksize_ok(p.ksize) && p.in && p.out;
  ok = ok && p.in_pitch >= (size_t)p.channels * p.W && p.out_pitch >= (size_t)p.channels * p.W && p.in_pitch <= 0xFFFFFFFFull / (size_t)p.H
       && p.out_pitch <= 0xFFFFFFFFull / (size_t)p.H && p.nstrips == blur_strips(p.W) && p.nchunks == blur_chunks(p.H)
       && (long long)p.total_items == (long long)p.nframes * p.nstrips * p.nchunks;
  // the levels: 1 .. K/2 + 1 of them, ascending within 0 .. K/2; every element row names one or is empty, and one is not
  ok = ok && p.nlevels >= 1 && p.nlevels <= p.ksize / 2 + 1;
  bool any = false;
  for (int l = 0; ok && l < p.nlevels; ++l) ok = p.level[l] >= (l ? p.level[l - 1] + 1 : 0) && p.level[l] <= p.ksize / 2;
  for (int j = 0; ok && j < p.ksize; ++j) {
    ok = p.row_level[j] >= -1 && p.row_level[j] < p.nlevels;
    any = any || p.row_level[j] >= 0;
  }
  if (!ok || !any) return hipErrorInvalidValue;
  const dim3 grid((p.total_items + 3) / 4), block(256);
  switch (p.ksize) {
  case 3: launch_k<3>(p, grid, block, s); break;
  case 5: launch_k<5>(p, grid, block, s); break;
  default: launch_k<7>(p, grid, block, s); break;
  }
  return hipGetLastError();
}

}  // namespace hc
