// corners.hip -- the kernels of hc_corner_response_device and hc_good_features_device: the Harris / smallest-eigenvalue measure of
// int16 derivative planes, and the strong, well-separated local maxima of a response plane (cv::cornerHarris / cv::cornerMinEigenVal
// and cv::goodFeaturesToTrack on the device; the contract is stated in include/hipcanny.h and restated in tests/corner_ref.py).
//
//   k_corner_response<B, METHOD>  the lane layout of k_deriv16: a wave owns a strip of 248 columns, lane l the 4 pixels at
//                   strip * 248 - 4 + 4 l, lanes 0 and 63 are halo.  The wave walks its chunk of rows downwards.  A lane keeps, for
//                   each of its 4 columns, the sums of dx^2, dx dy and dy^2 over the last B source rows as int64 (a product fits 32
//                   bits, seven of them do not): a new row adds its products and the row that leaves the window takes its own away
//                   again, from a register ring of the B raw rows -- 12 products in, 12 out, whatever B.  The window sum is
//                   separable: the B-column sums of the column sums come from the neighbouring lanes by DPP (two 32-bit moves a
//                   value), as a sliding window over 4 + 2 (B / 2) columns.  Rows replicate by clamping the row index, columns by
//                   clamping the column of each of a lane's elements.  No LDS, no atomics, no intermediate plane.
//                   Integer sums are exact, so their order cannot matter; the three conversions go int64 -> double (exact below
//                   2^53) -> float32 (one rounding), and every float step after them is one rounded operation.
//   k_feat_max      the largest key of each frame, over ALL its pixels: wave maxima, one integer atomicMax a wave.
//   k_feat_plane<MODE>  one text for the five walks over the plane that evaluate the candidate predicate (the pixel passes the
//                   threshold, lies in the interior and no neighbour has a larger key) from three rows of the plane:
//                   HIST: the candidates that agree with the cut key so far, counted by their next digit in an LDS histogram of the
//                         workgroup; its non-zero bins are added to the frame's histogram (integer sums: exact in any order);
//                   COUNT: the candidates with key > T and with key == T of each row -> rows[row];
//                   EMIT: (key, index) of every admitted candidate -> its slot: those above T from the row's offset on, the first
//                         `need` of the ties in raster order behind all of them (ballot + v_mbcnt, as k_edge_emit).
//   k_feat_walk     one wave per frame walks the histogram from the top bin down, 64 bins a trip: the next digit of T and how many
//                   candidates are still to admit below it; it leaves the histogram zeroed for the next pass.
//   k_feat_scan     one wave per frame: exclusive prefix sums over the rows' pairs in place, and the totals.
//   k_feat_rank     peak_rank (canny_device.h) on the unique (key, index): at most candidate_capacity records, so quadratic in that
//                   bound and in nothing else.  k_feat_sift: sift_min_distance (canny_device.h), the loop of k_circle_sift.
//   k_feat_out      the counts, the corners as (float x, float y) and their qualities.
// Every float step of the contract is one rounded float32 operation (__fmul_rn and its kin; this file is compiled with
// -ffp-contract=off, and says so itself below).
#include "canny_device.h"

#pragma clang fp contract(off)

namespace hc {

namespace {

typedef u32 u32x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ long long i64_from_lane_below(long long v)
{
  return (long long)(((u64)from_lane_below((u32)((u64)v >> 32)) << 32) | from_lane_below((u32)v));
}
static __device__ __forceinline__ long long i64_from_lane_above(long long v)
{
  return (long long)(((u64)from_lane_above((u32)((u64)v >> 32)) << 32) | from_lane_above((u32)v));
}
// one conversion of the exact integer, round to nearest even: |s| < 2^53 is exact as a double
static __device__ __forceinline__ float f32_of_sum(long long s) { return (float)(double)s; }

template <int METHOD>
static __device__ __forceinline__ float corner_measure(long long a, long long b, long long c, float k)
{
  const float fa = f32_of_sum(a), fb = f32_of_sum(b), fc = f32_of_sum(c);
  if constexpr (METHOD == CORNER_MIN_EIGEN) {
    const float h = __fmul_rn(0.5f, fa), g = __fmul_rn(0.5f, fc), d = __fsub_rn(h, g);
    // (__builtin_sqrtf: the correctly rounded root; __fsqrt_rn compiles to the bare v_sqrt_f32 here, which is good to 1 ulp only)
    return __fsub_rn(__fadd_rn(h, g), __builtin_sqrtf(__fadd_rn(__fmul_rn(d, d), __fmul_rn(fb, fb))));
  } else {
    const float t = __fadd_rn(fa, fc);
    return __fsub_rn(__fsub_rn(__fmul_rn(fa, fc), __fmul_rn(fb, fb)), __fmul_rn(__fmul_rn(k, t), t));
  }
}

template <int B, int METHOD>
__global__ __launch_bounds__(256) void k_corner_response(const CornerParams p)
{
  constexpr int R = B / 2, PX = CORNER_LANE_PX;
  const int lane = threadIdx.x & 63;
  const int item = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (int)(threadIdx.x >> 6));
  if (item >= p.total_items) return;
  const int chunk = item % p.nchunks;
  const int strip = (item / p.nchunks) % p.nstrips;
  const int frame = item / (p.nchunks * p.nstrips);
  const int W = p.W, H = p.H;
  const int r0 = chunk * CORNER_CHUNK_ROWS, rend = min(r0 + CORNER_CHUNK_ROWS, H);
  const int c0 = strip * CORNER_STRIP_W - PX + lane * PX;

  // The one place of the address arithmetic and of the replicated border: rows by clamping the row index, columns by clamping the
  // column of each element; a group that lies whole inside the row is read as one or two words where the planes are aligned that far
  int cc[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) cc[k] = min(max(c0 + k, 0), W - 1);
  const bool whole = c0 >= 0 && c0 + PX <= W;
  const int in_align = p.in_align;
  const uint8_t *const xbase = p.dx + (size_t)frame * p.frame_stride, *const ybase = p.dy + (size_t)frame * p.frame_stride;
  struct Raw { u32 x[2], y[2]; };  // packed int16 pairs: (px 0, px 1), (px 2, px 3)
  auto load_plane = [&](const uint8_t *rp, u32 (&w)[2]) {
    if (whole && in_align >= 8) {
      const u32x2v v = *reinterpret_cast<const u32x2v *>(rp + 2 * c0);
      w[0] = v.x; w[1] = v.y;
    } else if (whole && in_align >= 4) {
      w[0] = reinterpret_cast<const u32 *>(rp + 2 * c0)[0];
      w[1] = reinterpret_cast<const u32 *>(rp + 2 * c0)[1];
    } else {
      const unsigned short *h = reinterpret_cast<const unsigned short *>(rp);
      w[0] = (u32)h[cc[0]] | ((u32)h[cc[1]] << 16);
      w[1] = (u32)h[cc[2]] | ((u32)h[cc[3]] << 16);
    }
  };
  auto load_row = [&](int row) -> Raw {
    const u32 off = (u32)min(max(row, 0), H - 1) * (u32)p.pitch;  // (H * pitch < 2^32)
    Raw r;
    load_plane(xbase + off, r.x);
    load_plane(ybase + off, r.y);
    return r;
  };

  const bool st_lane = lane >= 1 && lane <= 62 && c0 < W;
  const bool st_full = c0 + PX <= W;
  const int out_align = p.out_align;
  uint8_t *const obase = p.out + (size_t)frame * p.out_frame_stride + 4 * (size_t)max(c0, 0);

  // column sums over the B source rows that ended with the last step: [a, b, c][column of the lane]
  long long S[3][PX];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int j = 0; j < PX; ++j) S[q][j] = 0;
  Raw ring[B];  // the raw rows inside the window; zeros (whose products are zeros) until B rows have arrived
#pragma unroll
  for (int u = 0; u < B; ++u) ring[u] = Raw{ { 0u, 0u }, { 0u, 0u } };

  // the 12 products of a raw row into S, added (the row arrives) or taken away (it leaves): one text for both, the sign a
  // compile-time tag so that each use is a plain chain of 64-bit adds or subtracts.  (The alternative -- a ring of B rows of
  // 32-bit products summed afresh per row -- saves the second set of multiplies for 12 (B - 1) more VGPRs and B - 1 adds a sum.)
  auto products = [&](const Raw &r, auto sign) {
    constexpr int sg = decltype(sign)::value;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const int x = (int)(short)(r.x[j >> 1] >> (16 * (j & 1))), y = (int)(short)(r.y[j >> 1] >> (16 * (j & 1)));
      // (|x|, |y| <= 2^15: each product lies in [-2^30 + 2^15, 2^30])
      S[0][j] += sg * (long long)(x * x);
      S[1][j] += sg * (long long)(x * y);
      S[2][j] += sg * (long long)(y * y);
    }
  };

  // one step: source row k arrives in ring slot u, the row k - B leaves -> output row g = k - R
  auto step = [&](auto uc, int k, const Raw &raw) {
    constexpr int u = decltype(uc)::value;
    products(ring[u], std::integral_constant<int, -1>{});
    products(raw, std::integral_constant<int, 1>{});
    ring[u] = raw;
    const int g = k - R;
    if (g < r0 || g >= rend) return;  // wave-uniform
    float out[PX];
    {
      long long acc[3][PX];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        // e[i]: the column sums of the columns c0 - R + i, i = 0 .. PX + 2 R - 1
        long long e[PX + 2 * R];
#pragma unroll
        for (int j = 0; j < PX; ++j) e[R + j] = S[q][j];
#pragma unroll
        for (int i = 0; i < R; ++i) {
          e[i] = i64_from_lane_below(S[q][PX - R + i]);
          e[R + PX + i] = i64_from_lane_above(S[q][i]);
        }
        long long w = 0;
#pragma unroll
        for (int i = 0; i < B; ++i) w += e[i];
        acc[q][0] = w;
#pragma unroll
        for (int j = 1; j < PX; ++j) {
          w += e[j + B - 1] - e[j - 1];
          acc[q][j] = w;
        }
      }
#pragma unroll
      for (int j = 0; j < PX; ++j) out[j] = corner_measure<METHOD>(acc[0][j], acc[1][j], acc[2][j], p.k);
    }
    if (!st_lane) return;
    uint8_t *q = obase + (u32)g * (u32)p.out_pitch;  // (H * out_pitch < 2^32)
    if (st_full && out_align >= 16) *reinterpret_cast<f32x4v *>(q) = f32x4v{ out[0], out[1], out[2], out[3] };
    else if (st_full && out_align >= 8) {
      reinterpret_cast<f32x2v *>(q)[0] = f32x2v{ out[0], out[1] };
      reinterpret_cast<f32x2v *>(q)[1] = f32x2v{ out[2], out[3] };
    } else {
#pragma unroll
      for (int j = 0; j < PX; ++j)
        if (c0 + j < W) reinterpret_cast<float *>(q)[j] = out[j];
    }
  };

  // source rows r0 - R .. rend - 1 + R, B steps per loop trip (the ring period); a row is requested B steps before it is used
  const int k0 = r0 - R, kend = rend + R;
  Raw bn[B];
#pragma unroll
  for (int j = 0; j < B; ++j) bn[j] = load_row(k0 + j);
  auto advance = [&](auto uc, int k) {
    constexpr int j = decltype(uc)::value;
    const Raw b = bn[j];
    bn[j] = load_row(k + B);
    step(uc, k, b);
  };
#pragma nounroll
  for (int k = k0; k < kend; k += B) {
    advance(std::integral_constant<int, 0>{}, k + 0);
    advance(std::integral_constant<int, 1>{}, k + 1);
    advance(std::integral_constant<int, 2>{}, k + 2);
    if constexpr (B > 3) {
      advance(std::integral_constant<int, 3>{}, k + 3);
      advance(std::integral_constant<int, 4>{}, k + 4);
    }
    if constexpr (B > 5) {
      advance(std::integral_constant<int, 5>{}, k + 5);
      advance(std::integral_constant<int, 6>{}, k + 6);
    }
  }
}

template <int B>
void launch_corner_block(const CornerParams &p, const dim3 grid, const dim3 block, hipStream_t s)
{
  if (p.method == CORNER_HARRIS) hipLaunchKernelGGL((k_corner_response<B, CORNER_HARRIS>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((k_corner_response<B, CORNER_MIN_EIGEN>), grid, block, 0, s, p);
}

// ---- hc_good_features_device ----------------------------------------------------------------------

static __device__ __forceinline__ const u32 *feat_row(const FeatParams &p, int frame, int row)
{
  return reinterpret_cast<const u32 *>(p.plane + (size_t)frame * p.frame_stride + (size_t)row * p.pitch);
}

__global__ __launch_bounds__(256) void k_feat_max(const FeatParams p)
{
  const int lane = threadIdx.x & 63;
  const int group = blockIdx.x, frame = blockIdx.y;
  const int r0 = group * FEAT_GROUP_ROWS, rend = min(r0 + FEAT_GROUP_ROWS, p.H);
  u32 m = 0;
  for (int row = r0 + (int)(threadIdx.x >> 6); row < rend; row += 4) {
    const u32 *rp = feat_row(p, frame, row);
    for (int x = lane; x < p.W; x += 64) m = max(m, feat_key(rp[x]));
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = max(m, (u32)__shfl_xor((int)m, off));
  if (lane == 0 && m) atomicMax(&p.state[(size_t)frame * FEAT_STATE_WORDS + FEAT_MAXKEY], m);
}

enum { FEAT_HIST0 = 0, FEAT_HIST1 = 1, FEAT_HIST2 = 2, FEAT_COUNT = 3, FEAT_EMIT = 4 };

template <int MODE>
__global__ __launch_bounds__(256) void k_feat_plane(const FeatParams p)
{
  constexpr bool HIST = MODE <= FEAT_HIST2;
  __shared__ u32 hist[HIST ? FEAT_BINS : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int group = blockIdx.x, frame = blockIdx.y;
  const int W = p.W, H = p.H;
  u32 *const st = p.state + (size_t)frame * FEAT_STATE_WORDS;
  const u32 all = st[FEAT_ALL], T = st[FEAT_T], need = st[FEAT_NEED], maxkey = st[FEAT_MAXKEY];  // uniform in the grid row
  if (HIST && MODE != FEAT_HIST0 && all) return;  // no cut: nothing to select
  if (HIST) {
    for (int i = threadIdx.x; i < FEAT_BINS; i += 256) hist[i] = 0u;
    __syncthreads();
  }
  // the threshold: t = M * q, one rounded product; a pixel passes iff key(v) > key(t)
  const u32 tkey = feat_key(__float_as_uint(__fmul_rn(__uint_as_float(maxkey), p.quality)));
  const int r0 = group * FEAT_GROUP_ROWS, rend = min(r0 + FEAT_GROUP_ROWS, H);
  u32 *const rows = p.rows + (size_t)frame * 2 * (size_t)H;
  const u32 cap = (u32)p.candidate_capacity;
  uint2 *const cand = reinterpret_cast<uint2 *>(p.cand) + (size_t)frame * cap;
  const u32 ngt = MODE == FEAT_EMIT ? st[FEAT_NGT] : 0u;

  // (a frame without a positive value: maxkey = tkey = 0 and every key is 0, so nothing passes; the tables are still written)
  for (int row = r0 + wave; row < rend; row += 4) {  // everything but `lane` is wave-uniform
    u32 n_gt = 0, n_eq = 0;                           // COUNT: of this row; EMIT: running offsets
    if (MODE == FEAT_EMIT) { n_gt = rows[2 * row]; n_eq = rows[2 * row + 1]; }
    if (row >= 1 && row <= H - 2) {
      const u32 *up = feat_row(p, frame, row - 1), *mid = feat_row(p, frame, row), *dn = feat_row(p, frame, row + 1);
      for (int x0 = 0; x0 + 2 < W; x0 += FEAT_TRIP_PX) {  // the lanes hold the columns x0 .. x0 + 63, the centres are x0 + 1 .. x0 + 62
        const int x = x0 + lane;
        u32 ku = 0, km = 0, kd = 0;
        if (x < W) { ku = feat_key(up[x]); km = feat_key(mid[x]); kd = feat_key(dn[x]); }
        const u32 col = max(max(ku, km), kd);  // the largest key of the column's three rows
        const u32 nb = max(max(from_lane_below(col), from_lane_above(col)), max(ku, kd));
        const bool is = lane >= 1 && lane <= 62 && x <= W - 2 && km > tkey && km >= nb;
        if constexpr (HIST) {
          if (is && feat_prefix(km, MODE) == feat_prefix(T, MODE)) atomicAdd(&hist[feat_digit(km, MODE)], 1u);
        } else {
          const bool gt = is && km > T, eq = is && km == T;
          const u64 mg = __ballot(gt), me = __ballot(eq);
          if constexpr (MODE == FEAT_EMIT) {
            const u32 index = (u32)row * (u32)W + (u32)x;
            if (gt) {
              const u32 slot = n_gt + mbcnt64(mg);
              if (slot < cap) cand[slot] = make_uint2(km, index);
            }
            if (eq) {
              const u32 tie = n_eq + mbcnt64(me);  // the tie's number in raster order
              if (tie < need && ngt + tie < cap) cand[ngt + tie] = make_uint2(km, index);
            }
          }
          n_gt += (u32)__popcll(mg);
          n_eq += (u32)__popcll(me);
        }
      }
    }
    if (MODE == FEAT_COUNT && lane == 0) { rows[2 * row] = n_gt; rows[2 * row + 1] = n_eq; }
  }
  if (HIST) {
    __syncthreads();
    u32 *const gh = p.hist + (size_t)frame * FEAT_BINS;
    for (int i = threadIdx.x; i < FEAT_BINS; i += 256)
      if (const u32 v = hist[i]) atomicAdd(&gh[i], v);
  }
}

// After pass `pass`: T holds the digits fixed so far, NEED the candidates still to admit among those that agree with T (after the
// last pass: the ties admitted).  Pass 0 starts from need = candidate_capacity; a frame with no more candidates than that is
// marked ALL, with T = 0 (every candidate's key is above 0).
__global__ __launch_bounds__(64) void k_feat_walk(const FeatParams p, const int pass)
{
  const int lane = threadIdx.x, frame = blockIdx.x;
  u32 *const st = p.state + (size_t)frame * FEAT_STATE_WORDS;
  u32 *const gh = p.hist + (size_t)frame * FEAT_BINS;
  if (pass > 0 && st[FEAT_ALL]) return;
  const u32 need = pass == 0 ? (u32)p.candidate_capacity : st[FEAT_NEED];
  u32 above = 0;  // candidates in the bins above this trip's: wave-uniform
  bool found = false;
  u32 digit = 0, above_digit = 0;
  for (int b0 = FEAT_BINS - 64; b0 >= 0; b0 -= 64) {
    const int bin = b0 + 63 - lane;  // lane 0 holds the trip's top bin
    const u32 v = gh[bin];
    gh[bin] = 0u;
    u32 incl = v;  // candidates of this trip's bins >= mine
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (!found) {
      const u64 m = __ballot(above + incl >= need);  // the first such lane holds the digit
      if (m) {
        const int l = __builtin_ctzll(m);
        digit = (u32)(b0 + 63 - l);
        above_digit = above + (u32)__shfl((int)(incl - v), l);
        found = true;
      }
    }
    above += (u32)__shfl((int)incl, 63);
  }
  if (lane != 0) return;
  if (!found) {  // fewer candidates than are wanted (pass 0 only: later passes walk a class that holds `need` at least)
    st[FEAT_ALL] = 1u; st[FEAT_T] = 0u; st[FEAT_NEED] = 0u;
    return;
  }
  st[FEAT_T] = (pass == 0 ? 0u : st[FEAT_T]) | (digit << feat_shift(pass));
  st[FEAT_NEED] = need - above_digit;
}

__global__ __launch_bounds__(64) void k_feat_scan(const FeatParams p)
{
  const int lane = threadIdx.x, frame = blockIdx.x;
  u32 *const st = p.state + (size_t)frame * FEAT_STATE_WORDS;
  u32 *const rows = p.rows + (size_t)frame * 2 * (size_t)p.H;
  u32 cg = 0, ce = 0;
  for (int r0 = 0; r0 < p.H; r0 += 64) {
    const int r = r0 + lane;
    const u32 vg = r < p.H ? rows[2 * r] : 0u, ve = r < p.H ? rows[2 * r + 1] : 0u;
    u32 ig = vg, ie = ve;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 tg = __shfl_up(ig, off), te = __shfl_up(ie, off);
      if (lane >= off) { ig += tg; ie += te; }
    }
    if (r < p.H) { rows[2 * r] = cg + ig - vg; rows[2 * r + 1] = ce + ie - ve; }
    cg += __shfl(ig, 63);
    ce += __shfl(ie, 63);
  }
  if (lane == 0) {
    st[FEAT_NGT] = cg;
    st[FEAT_NCAND] = min(cg + min(ce, st[FEAT_NEED]), (u32)p.candidate_capacity);
  }
}

__global__ __launch_bounds__(HOUGH_RANK_THREADS) void k_feat_rank(const FeatParams p)
{
  __shared__ uint2 tile[HOUGH_RANK_THREADS];
  const int frame = blockIdx.y;
  const u32 np = p.state[(size_t)frame * FEAT_STATE_WORDS + FEAT_NCAND];  // uniform in the workgroup
  const u32 i0 = blockIdx.x * HOUGH_RANK_THREADS;
  if (i0 >= np) return;
  const uint2 *pk = reinterpret_cast<const uint2 *>(p.cand) + (size_t)frame * p.candidate_capacity;
  const u32 i = i0 + threadIdx.x;
  const uint2 me = i < np ? pk[i] : make_uint2(0u, 0u);
  const u32 rank = peak_rank(pk, np, me, tile);  // key descending, index ascending
  if (i >= np) return;
  reinterpret_cast<int4 *>(p.ranked)[(size_t)frame * p.candidate_capacity + rank] = make_int4((int)me.x, (int)(me.y % (u32)p.W), (int)(me.y / (u32)p.W), 0);
}

__global__ __launch_bounds__(64) void k_feat_sift(const FeatParams p)
{
  __shared__ int2 kept_xy[FEAT_MAX_CANDIDATES];
  const int frame = blockIdx.x;
  u32 *const st = p.state + (size_t)frame * FEAT_STATE_WORDS;
  const u32 nc = min(st[FEAT_NCAND], (u32)p.candidate_capacity);
  const int4 *in = reinterpret_cast<const int4 *>(p.ranked) + (size_t)frame * p.candidate_capacity;
  int4 *out = reinterpret_cast<int4 *>(p.kept) + (size_t)frame * p.candidate_capacity;
  const u32 nk = sift_min_distance(in, nc, p.min_d2, kept_xy, out);
  if (threadIdx.x == 0) st[FEAT_NKEPT] = nk;
}

__global__ __launch_bounds__(256) void k_feat_out(const FeatParams p)
{
  const int frame = blockIdx.x;
  const u32 nk = p.state[(size_t)frame * FEAT_STATE_WORDS + FEAT_NKEPT];
  if (threadIdx.x == 0) p.counts[frame] = nk;
  const u32 n = (u32)min((size_t)nk, p.corner_capacity);
  const int4 *kept = reinterpret_cast<const int4 *>(p.kept) + (size_t)frame * p.candidate_capacity;
  for (u32 i = threadIdx.x; i < n; i += 256) {
    const int4 c = kept[i];
    reinterpret_cast<f32x2v *>(p.corners)[(size_t)frame * p.corner_capacity + i] = f32x2v{ (float)c.y, (float)c.z };
    if (p.quality_out) reinterpret_cast<u32 *>(p.quality_out)[(size_t)frame * p.corner_capacity + i] = (u32)c.x;  // the response, bit for bit
  }
}

}  // namespace

hipError_t launch_corner_response(const CornerParams &p, hipStream_t s)
{
  const uintptr_t ia = (uintptr_t)p.dx | (uintptr_t)p.dy | p.pitch | p.frame_stride, oa = (uintptr_t)p.out | p.out_pitch | p.out_frame_stride;
  if (p.W < 1 || p.H < 1 || p.nframes < 1 || !p.dx || !p.dy || !p.out || !corner_block_ok(p.block_size) || (p.method != CORNER_MIN_EIGEN && p.method != CORNER_HARRIS)
      || (p.in_align != 8 && p.in_align != 4 && p.in_align != 2) || (ia & (uintptr_t)(p.in_align - 1)) || (p.out_align != 16 && p.out_align != 8 && p.out_align != 4)
      || (oa & (uintptr_t)(p.out_align - 1)) || p.pitch < 2 * (size_t)p.W || p.out_pitch < 4 * (size_t)p.W || (unsigned long long)p.H * p.pitch >= (1ull << 32)
      || (unsigned long long)p.H * p.out_pitch >= (1ull << 32) || p.nstrips != corner_strips(p.W) || p.nchunks != corner_chunks(p.H)
      || (long long)p.total_items != (long long)p.nframes * p.nstrips * p.nchunks)
    return hipErrorInvalidValue;
  const dim3 grid((p.total_items + 3) / 4), block(256);
  switch (p.block_size) {
  case 3: launch_corner_block<3>(p, grid, block, s); break;
  case 5: launch_corner_block<5>(p, grid, block, s); break;
  default: launch_corner_block<7>(p, grid, block, s); break;
  }
  return hipGetLastError();
}

// One pass on stream s, behind the zeroing of p.hist and p.state.  corner_capacity == 0: counts only (p.corners is not looked at).
hipError_t launch_good_features(const FeatParams &p, hipStream_t s)
{
  if (!p.plane || !p.counts || !p.ranked || !p.kept || !p.cand || !p.hist || !p.state || !p.rows || (((uintptr_t)p.plane | p.pitch | p.frame_stride) & 3u)
      || (((uintptr_t)p.counts | (uintptr_t)p.hist | (uintptr_t)p.state | (uintptr_t)p.rows | (uintptr_t)p.quality_out) & 3u) || (((uintptr_t)p.cand | (uintptr_t)p.corners) & 7u)
      || (((uintptr_t)p.ranked | (uintptr_t)p.kept) & 15u) || p.W < 1 || p.H < 1 || p.nframes < 1 || p.nframes > 65535 || p.pitch < 4 * (size_t)p.W
      || (unsigned long long)p.H * p.pitch >= (1ull << 32) || p.ngroups != feat_groups(p.H) || p.candidate_capacity < 1 || p.candidate_capacity > FEAT_MAX_CANDIDATES
      || p.min_d2 < 0 || (p.corner_capacity && !p.corners))
    return hipErrorInvalidValue;
  const unsigned n = (unsigned)p.nframes;
  const dim3 plane_grid((unsigned)p.ngroups, n), block(256);
  hipLaunchKernelGGL(k_feat_max, plane_grid, block, 0, s, p);
  hipLaunchKernelGGL(k_feat_plane<FEAT_HIST0>, plane_grid, block, 0, s, p);
  hipLaunchKernelGGL(k_feat_walk, dim3(n), dim3(64), 0, s, p, 0);
  hipLaunchKernelGGL(k_feat_plane<FEAT_HIST1>, plane_grid, block, 0, s, p);
  hipLaunchKernelGGL(k_feat_walk, dim3(n), dim3(64), 0, s, p, 1);
  hipLaunchKernelGGL(k_feat_plane<FEAT_HIST2>, plane_grid, block, 0, s, p);
  hipLaunchKernelGGL(k_feat_walk, dim3(n), dim3(64), 0, s, p, 2);
  hipLaunchKernelGGL(k_feat_plane<FEAT_COUNT>, plane_grid, block, 0, s, p);
  hipLaunchKernelGGL(k_feat_scan, dim3(n), dim3(64), 0, s, p);
  hipLaunchKernelGGL(k_feat_plane<FEAT_EMIT>, plane_grid, block, 0, s, p);
  hipLaunchKernelGGL(k_feat_rank, dim3((unsigned)((p.candidate_capacity + HOUGH_RANK_THREADS - 1) / HOUGH_RANK_THREADS), n), dim3(HOUGH_RANK_THREADS), 0, s, p);
  hipLaunchKernelGGL(k_feat_sift, dim3(n), dim3(64), 0, s, p);
  hipLaunchKernelGGL(k_feat_out, dim3(n), block, 0, s, p);
  return hipGetLastError();
}

}  // namespace hc
