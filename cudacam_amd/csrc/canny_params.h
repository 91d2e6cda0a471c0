// canny_params.h -- the parameter blocks the host hands to the kernels and the geometry facts it plans with.
// Plain C++ (no HIP): shared by the kernel files, the launcher (hipcanny.hip), the planner (host_plan.h) and the CPU test
// of the planner.  Every kernel constant the host also needs is defined here, once.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hc {

typedef uint32_t u32;
typedef uint64_t u64;

// ---- geometry of the fused path ---------------------------------------------------------------
// A wave owns a vertical STRIP of the frame: lane l holds the 4 adjacent pixels at columns
// strip*STRIP_W - 4 + 4*l .. +3 of the current row, packed in one dword.  Lanes 0 and 63 are halo
// lanes (4 px each side = 2 blur + 1 Sobel + 1 NMS), lanes 1..62 produce STRIP_W = 248 outputs.
constexpr int LANES = 64;
constexpr int PX_PER_LANE = 4;
constexpr int STRIP_W = (LANES - 2) * PX_PER_LANE;  // 248
constexpr int STRIP_HALO = PX_PER_LANE;             // 4 columns = one lane

// Bit planes: two plain bitmaps per frame, STRONG and CANDIDATE (candidate includes strong):
// bit c of a row <-> column c, rows padded to RD dwords.  A strip's 248 valid columns are 31 whole
// bytes, so each wave-row of k_front stores its 31 bytes at byte offset strip*31 of the row.
struct FrontParams {
  const uint8_t *in;       // u8 frames, pitched: mono, or interleaved BGR when bgr != 0 (stage 0 fused into the load)
  int bgr;
  size_t in_pitch;         // bytes per row   (multiple of 4)
  size_t in_frame_stride;  // bytes per frame (multiple of 4)
  u32 *sbits, *cbits;      // bit planes [frame][H][RD]
  int RD;                  // dwords per bit-plane row
  int W, H;
  int nstrips, nchunks, nframes;
  int subchunks;   // k_front (legacy_front.hip) only: sub-chunks of 24 blur rows a wave marches through per work item
  int run_rows;    // the run-based kernels (k_front8 / k_front8o, k_front_mx, k_front, k_blur): output rows per work item; nchunks = ceil(H / run_rows).  k_front: = 24 * subchunks - 4
  int chunk_rows;          // Mode O kernel: output rows per work item (any value >= 1)
  int l2gradient;          // Mode O kernel: magnitude dx^2 + dy^2 instead of |dx| + |dy| (cv::Canny's L2gradient)
  int total_items;         // nframes * nstrips * nchunks
  // thresholds on S = sumX^2 + sumY^2 for "u8-wrapped gradient > T" (band test)
  u32 a_lo[3], a_hi[3];
  // split mode (k_blur + k_nms, legacy_front.hip): the u8 blur plane between the two kernels -- k_blur writes it by
  // nchunks / run_rows / total_items, k_nms reads it by its own work split
  uint8_t *blur;             // k_blur, k_nms: [frame][strip][H][256]: one aligned 256-byte row per wave-row (bytes 4..251 = the strip's columns)
  size_t blur_frame_stride;  // >= nstrips * H * 256
  int nchunks_b, run_rows_b, total_items_b;  // k_nms only
  // k_nms: when set, the strong pixels are also written as 255 (others 0) into this u8 map -- the provisional edge
  // map the hysteresis then only patches (W % 4 == 0: a lane stores its 4 pixels as one dword)
  uint8_t *prov_out; u32 prov_pitch; size_t prov_fs;
  // diagnostics (HC_OPT_DEBUG_TAPS): the fused kernel also stores its (fixed-up) blur rows here, plain [frame][H][pitch]
  uint8_t *dbg_blur; u32 dbg_pitch; size_t dbg_fs;
  const uint8_t *zeros;  // k_front8: >= 3 * 8192 + 32 bytes of zeros (what rows above / below the image read as); HALF form: + in_frame_stride
  // k_front8: memory that may be overwritten with anything -- where the branch-free row code stores rows that are not its
  // own: STRONG plane bytes (dump), CANDIDATE plane bytes (dump_c), provisional map (dump_p).  Plain form: 2 KiB, 2 KiB,
  // W + 8 bytes.  HALF form: each + the byte offset of half-wave B's frame (3 * H * RD * 4 / 3 * prov_fs at most).
  uint8_t *dump, *dump_c, *dump_p;
  // k_front8 / k_front8o: words the kernel zeroes before anything else (the run's hysteresis flags, worklist counts and
  // reason words: one memset kernel and one host call fewer per run); null: nothing
  u32 *zero_words; u32 zero_count;
  int half;        // k_front8: HALF form (two 240-column half-strips per wave, narrow frames); nstrips is unused then
  int one_wave;    // k_front8, mono / BGR with a provisional map: one-wave workgroups instead of four-wave ones
  int nhalf;       // HALF form: half-strips per frame = ceil(W / 240); total_items = ceil(in_frames * nhalf / 2) * nchunks (* 3 per-channel)
  // k_front8: a window that follows one with more than dense_enter half-lanes above the low threshold takes the dense path
  // (wave-wide NMS in registers), and the windows after it while they count more than dense_leave (0x7FFFFFFF: never)
  int dense_enter, dense_leave;
  u32 wrap_limit;  // S >= wrap_limit: gradient >= 256, the wrap bands apply (0xFFFFFFFF: saturating variant)
  // Mode O (k_front_o, k_front8o, k_front_o_ext at aperture 5 / on given gradients): null, or int32 [nframes][2] = (low, high)
  // per frame in the units of hc_set_thresholds (hc_frame_thresholds_device) -- frame f is then cut with
  // frame_threshold_pair(frame_thr[2f], frame_thr[2f + 1]) (below; on the device through frame_thresholds, canny_device.h) instead
  // of a_lo[0] / a_hi[0], by the kernels' TAB instantiations, which their launchers pick when it is set.  A device pointer the launcher
  // patches in: no plan sets it
  const int32_t *frame_thr;
};

#if defined(__HIPCC__)
#define HC_HOST_DEVICE __host__ __device__
#else
#define HC_HOST_DEVICE
#endif
// One (low, high) pair of a per-frame table as the Mode O kernels compare it: what hc_set_thresholds followed by
// plan_thresholds_and_masks (host_plan.h) make of the same pair for a context -- clamped to 0..32767, ordered, squared
// for L2gradient (32767^2 < 2^31).  The kernels call it per work item, the CPU test on a grid of pairs.
HC_HOST_DEVICE inline void frame_threshold_pair(int low, int high, int l2gradient, u32 *a_lo, u32 *a_hi)
{
  low = low < 0 ? 0 : low > 32767 ? 32767 : low;
  high = high < 0 ? 0 : high > 32767 ? 32767 : high;
  const int lo = low > high ? high : low, hi = low > high ? low : high;
  *a_lo = l2gradient ? (u32)lo * (u32)lo : (u32)lo;
  *a_hi = l2gradient ? (u32)hi * (u32)hi : (u32)hi;
}

// Mode O beyond k_front_o (front_o_ext.hip): the 5x5 / 7x7 Sobel or the Scharr derivatives of u8 frames (apertures 5, 7,
// -1), or caller-given int16 derivatives (cv::Canny's (dx, dy) overload).  f as for k_front_o (thresholds in a_lo[0] /
// a_hi[0], chunk_rows, l2gradient); with gradients != 0, f.in is dx and dy the dy planes, both with f.in_pitch /
// f.in_frame_stride (bytes, even), `channels` interleaved int16 per pixel.
struct FrontExtParams {
  FrontParams f;
  int gradients;
  int channels;
  const uint8_t *dy;
  int aperture = 5;  // gradients == 0: the kind of the u8 source, 5, 7 (sums / 16, half to even) or -1 (Scharr)
};

// k_deriv16 (deriv.hip): the Sobel / Scharr derivatives cv::Canny computes before its NMS, u8 frames -> int16 dx / dy planes
// with the input's channel interleave.  Strips and lanes as the 4-px front kernels (one halo lane = 4 columns each side; the
// 7-tap filters need 3); a work item is (frame, strip, DERIV_CHUNK_ROWS output rows) with a warm-up of ksize - 1 rows.
constexpr int DERIV_STRIP_W = 248;       // output columns per wave
static_assert(DERIV_STRIP_W == STRIP_W, "k_deriv16 uses the lane layout of the 4-px front kernels");
constexpr int DERIV_CHUNK_ROWS = 64;     // output rows per work item
constexpr bool deriv_ksize_ok(int ksize) { return ksize == 3 || ksize == 5 || ksize == 7 || ksize == -1; }
inline int deriv_strips(int W) { return (W + DERIV_STRIP_W - 1) / DERIV_STRIP_W; }
inline int deriv_chunks(int H) { return (H + DERIV_CHUNK_ROWS - 1) / DERIV_CHUNK_ROWS; }
struct DerivParams {
  const uint8_t *in;       // u8 frames, `channels` interleaved; any alignment (in_aligned: base, pitch and frame stride are multiples of 4)
  size_t in_pitch, in_frame_stride;
  uint8_t *dx, *dy;        // int16 planes, even addresses; same pitch / frame stride (bytes, even)
  size_t pitch, frame_stride;
  int W, H, nframes, channels;
  int ksize;               // 3, 5, 7 (scaled by 1/16, rounded half to even) or -1 (Scharr)
  int in_aligned;          // the input rows may be read as dwords (whole 4-pixel groups inside the row only)
  int out_align;           // 8, 4 or 2: what base, pitch and frame stride of BOTH outputs are multiples of
  int nstrips, nchunks, total_items;
};

// k_gauss8 (blur.hip): a separable K x K smoothing filter with Q8 taps, u8 frames -> u8 frames of the same interleave
// (hc_gaussian_blur_device, where the arithmetic is stated).  Strips, lanes and chunks as k_deriv16.
constexpr int BLUR_STRIP_W = 248;        // output columns per wave
static_assert(BLUR_STRIP_W == STRIP_W, "k_gauss8 uses the lane layout of the 4-px front kernels");
constexpr int BLUR_CHUNK_ROWS = 64;      // output rows per work item
constexpr int BLUR_MAX_TAPS = 7;
constexpr int BLUR_REFLECT_101 = 0, BLUR_REPLICATE = 1;  // HC_BORDER_* (host_plan.h asserts the match)
constexpr bool blur_ksize_ok(int ksize) { return ksize == 3 || ksize == 5 || ksize == 7; }
inline int blur_strips(int W) { return (W + BLUR_STRIP_W - 1) / BLUR_STRIP_W; }
inline int blur_chunks(int H) { return (H + BLUR_CHUNK_ROWS - 1) / BLUR_CHUNK_ROWS; }
// cv::borderInterpolate for the two borders: index i of an axis of n >= 1 elements, clamped (BLUR_REPLICATE) or reflected
// about the edge elements without repeating them, until it lies inside (BLUR_REFLECT_101; n == 1: 0).  The kernel calls it
// for indices within 3 of the axis, the CPU tests for any.
HC_HOST_DEVICE inline int border_index(int i, int n, int border)
{
  if (border == BLUR_REPLICATE) return i < 0 ? 0 : i >= n ? n - 1 : i;
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}
struct BlurParams {
  const uint8_t *in;       // u8 frames, `channels` interleaved; any alignment (in_aligned: base, pitch and frame stride are multiples of 4)
  size_t in_pitch, in_frame_stride;
  uint8_t *out;            // u8 frames of the same shape; any alignment (out_aligned as in_aligned); no byte shared with the input view
  size_t out_pitch, out_frame_stride;
  int W, H, nframes, channels;
  int ksize;               // 3, 5 or 7
  int border;              // BLUR_REFLECT_101 or BLUR_REPLICATE
  int in_aligned;          // the input rows may be read as dwords (whole 4-pixel groups inside the row only)
  int out_aligned;         // the output rows may be written as dwords (likewise)
  int nstrips, nchunks, total_items;
  uint16_t taps[BLUR_MAX_TAPS + 1];  // Q8 (256 = 1.0), each <= 256, sum 256; [ksize ..]: 0
};

// k_morph8 (morph.hip): one launch of a K x K maximum (dilate) or, on complemented bytes, minimum (erode) filter, u8 frames -> u8
// frames of the same interleave (hc_morphology_device, where the operation is stated).  Strips, lanes and chunks as k_gauss8.
// The element is K half-widths per row; the kernel keeps one horizontal maximum per DISTINCT half-width (a "level") of each of the
// last K rows, so the plan hands it the levels (ascending) and, per element row, the index of its level.
constexpr int MORPH_MAX_K = 7, MORPH_MAX_LEVELS = 4;  // (half-widths 0 .. 3)
constexpr int MORPH_ERODE = 0, MORPH_DILATE = 1, MORPH_OPEN = 2, MORPH_CLOSE = 3, MORPH_GRADIENT = 4;  // HC_MORPH_* (host_plan.h asserts the match)
struct MorphParams {
  const uint8_t *in;       // u8 frames, `channels` interleaved; any alignment (in_aligned: base, pitch and frame stride are multiples of 4)
  size_t in_pitch, in_frame_stride;
  uint8_t *out;            // u8 frames of the same shape; any alignment (out_aligned as in_aligned); no byte shared with the input view
  size_t out_pitch, out_frame_stride;
  int W, H, nframes, channels;
  int ksize;               // 3, 5 or 7
  int complement;          // 1: bytes are complemented after the load and before the store -- the maximum filter erodes
  int subtract;            // 1: out = (what out holds) - result, bytewise (the second launch of GRADIENT; the result never exceeds it)
  int in_aligned, out_aligned;  // as BlurParams
  int nstrips, nchunks, total_items;
  int nlevels;                      // 1 .. ksize / 2 + 1 distinct half-widths
  int8_t level[MORPH_MAX_LEVELS];   // ... ascending; [nlevels ..]: 0
  int8_t row_level[MORPH_MAX_K + 1];  // per element row: the index of its half-width in level[], -1: an empty row; [ksize ..]: -1
};

// k_thin_pack / k_thin_step / k_thin_unpack (thin.hip): Zhang-Suen and Guo-Hall thinning of binary maps on bit planes
// (hc_thinning_device, where the rules are stated).  A plane holds a frame as H rows of thin_row_words(W) dwords, bit i of word j =
// column 32 j + i; the bits beyond W are zero.  A lane of k_thin_step holds one dword of a row, so a wave spans a panel of
// THIN_PANEL_WORDS words (2048 columns); a work item is (frame, panel, tile of THIN_TILE_ROWS rows), one per wave, four to a
// workgroup.  16 rows: 1080p x 64 frames are 4352 waves, four to a SIMD, for one halo row in eight read twice.
constexpr int THIN_ZHANGSUEN = 0, THIN_GUOHALL = 1;  // HC_THIN_* (host_plan.h asserts the match)
constexpr int THIN_MAX_ITERATIONS = 1024;
constexpr int THIN_TILE_ROWS = 16;
constexpr int THIN_PANEL_WORDS = 64;
constexpr int THIN_SEG_PX = 256;  // columns a wave of k_thin_pack / k_thin_unpack covers: 4 per lane, 8 words
inline int thin_row_words(int W) { return (W + 31) / 32; }
inline int thin_panels(int W) { return (thin_row_words(W) + THIN_PANEL_WORDS - 1) / THIN_PANEL_WORDS; }
inline int thin_tiles(int H) { return (H + THIN_TILE_ROWS - 1) / THIN_TILE_ROWS; }
inline int thin_segs(int W) { return (W + THIN_SEG_PX - 1) / THIN_SEG_PX; }
// The scratch of a pass of F frames: [plane A x F][plane B x F][removal table x F].  A frame's table holds table_words =
// max_iterations + 1 words: word k (1 ..) is the number of pixels iteration k removed, word 0 is not used.
struct ThinPackParams {
  const uint8_t *map;      // u8 maps of W x H, one channel, any alignment (in_aligned: base, pitch and frame stride are multiples of 4)
  size_t pitch, frame_stride;
  u32 *plane_a;            // [nframes][H][row_words]
  size_t plane_words;      // H * row_words
  int W, H, nframes, row_words, segs;
  int in_aligned;          // rows may be read as dwords (whole 4-pixel groups inside the row only)
};
struct ThinStepParams {
  u32 *plane_a, *plane_b;  // sub-iteration 0 reads A and writes B, sub-iteration 1 reads B and writes A
  u32 *removed;            // [nframes][table_words]; zero when the first step starts
  size_t plane_words;
  int H, nframes, row_words, npanels, ntiles, total_items;  // total_items = nframes * npanels * ntiles
  int table_words;
  int method;              // THIN_ZHANGSUEN / THIN_GUOHALL
};
struct ThinUnpackParams {
  const u32 *plane_a;
  const u32 *removed;
  u32 *status;             // [nframes][2] = (iterations that removed a pixel, 1: the fixed point was reached), or null
  uint8_t *out;            // u8 maps 0 / 255; any alignment (out_aligned as in_aligned); exactly [row, row + W) is written
  size_t out_pitch, out_frame_stride;
  size_t plane_words;
  int W, H, nframes, row_words, segs;
  int out_aligned;
  int table_words, max_iterations;
};
// The bit-sliced decision of k_thin_step, plain C++ on dwords so that the CPU test can run the kernel's own text against the
// per-pixel formulas (tests/cpp/thin_plan_driver.cpp).  A row as three planes: the row, its west-neighbour plane (pixel x - 1 at
// bit x) and its east-neighbour plane.
struct ThinRow { u32 c, w, e; };
// exactly-one accumulator over planes: `one` = at least one seen, `more` = at least two
struct ThinOneOf {
  u32 one = 0, more = 0;
  HC_HOST_DEVICE inline void add(u32 t) { more |= one & t; one |= t; }
  HC_HOST_DEVICE inline u32 exactly_one() const { return one & ~more; }
};
// the pixels of row C that sub-iteration S of METHOD removes (N, S_: the rows above and below): include/hipcanny.h states the rules
template <int METHOD, int S>
HC_HOST_DEVICE inline u32 thin_removed(const ThinRow &N, const ThinRow &C, const ThinRow &S_)
{
  const u32 p2 = N.c, p3 = N.e, p4 = C.e, p5 = S_.e, p6 = S_.c, p7 = S_.w, p8 = C.w, p9 = N.w;
  if constexpr (METHOD == THIN_ZHANGSUEN) {
    // B = p2 + .. + p9 as a carry-save count: bits b0 .. b3
    const u32 s1 = p2 ^ p3 ^ p4, c1 = (p2 & p3) | (p4 & (p2 ^ p3));
    const u32 s2 = p5 ^ p6 ^ p7, c2 = (p5 & p6) | (p7 & (p5 ^ p6));
    const u32 s3 = p8 ^ p9, c3 = p8 & p9;
    const u32 b0 = s1 ^ s2 ^ s3, c4 = (s1 & s2) | (s3 & (s1 ^ s2));
    const u32 s5 = c1 ^ c2 ^ c3, c5 = (c1 & c2) | (c3 & (c1 ^ c2));
    const u32 b1 = s5 ^ c4, c6 = s5 & c4;
    const u32 b2 = c5 ^ c6, b3 = c5 & c6;
    const u32 b_ok = (b1 | b2) & ~b3 & ~(b2 & b1 & b0);  // 2 <= B <= 6
    ThinOneOf a;  // A: the 0 -> 1 steps of the cyclic sequence p2, p3, .., p9, p2
    a.add(~p2 & p3); a.add(~p3 & p4); a.add(~p4 & p5); a.add(~p5 & p6);
    a.add(~p6 & p7); a.add(~p7 & p8); a.add(~p8 & p9); a.add(~p9 & p2);
    const u32 cond = S == 0 ? ~(p2 & p4 & p6) & ~(p4 & p6 & p8) : ~(p2 & p4 & p8) & ~(p2 & p6 & p8);
    return C.c & b_ok & a.exactly_one() & cond;
  } else {
    ThinOneOf c;
    c.add(~p2 & (p3 | p4)); c.add(~p4 & (p5 | p6)); c.add(~p6 & (p7 | p8)); c.add(~p8 & (p9 | p2));
    const u32 a1 = p9 | p2, a2 = p3 | p4, a3 = p5 | p6, a4 = p7 | p8;  // N1 = a1 + a2 + a3 + a4
    const u32 d1 = p2 | p3, d2 = p4 | p5, d3 = p6 | p7, d4 = p8 | p9;  // N2 likewise
    ThinOneOf n1, n2;
    n1.add(a1); n1.add(a2); n1.add(a3); n1.add(a4);
    n2.add(d1); n2.add(d2); n2.add(d3); n2.add(d4);
    // 2 <= min(N1, N2) <= 3: both counts reach 2, and not both are 4
    const u32 n_ok = n1.more & n2.more & ~(a1 & a2 & a3 & a4 & d1 & d2 & d3 & d4);
    const u32 m = S == 0 ? (p6 | p7 | ~p9) & p8 : (p2 | p3 | ~p5) & p4;
    return C.c & c.exactly_one() & n_ok & ~m;
  }
}

// k_corner_response (corners.hip): the Harris / smallest-eigenvalue measure of one-channel int16 derivative planes
// (hc_corner_response_device, where the arithmetic is stated).  The lane layout of k_deriv16: a wave owns a strip of
// CORNER_STRIP_W columns, lane l the 4 pixels at strip * CORNER_STRIP_W - 4 + 4 l, lanes 0 and 63 are halo (4 >= block_size / 2
// columns); a work item is (frame, strip, CORNER_CHUNK_ROWS output rows) with a warm-up of block_size - 1 rows.
constexpr int CORNER_MIN_EIGEN = 0, CORNER_HARRIS = 1;  // HC_CORNER_* (host_plan.h asserts the match)
constexpr int CORNER_STRIP_W = 248;
constexpr int CORNER_LANE_PX = 4;
constexpr int CORNER_CHUNK_ROWS = 64;
inline bool corner_block_ok(int b) { return b == 3 || b == 5 || b == 7; }
inline int corner_strips(int W) { return (W + CORNER_STRIP_W - 1) / CORNER_STRIP_W; }
inline int corner_chunks(int H) { return (H + CORNER_CHUNK_ROWS - 1) / CORNER_CHUNK_ROWS; }
struct CornerParams {
  const uint8_t *dx, *dy;  // int16 planes of W x H, one channel; one pitch and one frame stride (bytes, even)
  size_t pitch, frame_stride;
  uint8_t *out;            // float32 planes of W x H; exactly [row, row + 4 W) of a row is written
  size_t out_pitch, out_frame_stride;
  int W, H, nframes;
  int block_size, method;  // 3 / 5 / 7; CORNER_MIN_EIGEN / CORNER_HARRIS
  float k;                 // (float)harris_k; 0 with CORNER_MIN_EIGEN
  int in_align;            // 8 / 4 / 2: what both bases, the pitch and the frame stride are multiples of
  int out_align;           // 16 / 8 / 4 likewise
  int nstrips, nchunks, total_items;  // total_items = nframes * nstrips * nchunks
};

// The kernels of hc_good_features_device (corners.hip).  A key is the bit pattern of a response v > 0, else 0 (feat_key): keys
// order as the values do, so every comparison is an integer one.  The cut at candidate_capacity is an exact radix select on the
// key, FEAT_PASSES passes of FEAT_BINS bins at most, from the top digit down (feat_digit).
// k_feat_plane: a workgroup of 4 waves takes FEAT_GROUP_ROWS rows of a frame, wave w the rows r0 + w, r0 + w + 4, ..; in a row a
// trip covers FEAT_TRIP_PX centre columns with the lanes 1 .. 62, lanes 0 and 63 hold the neighbour columns.
constexpr int FEAT_MAX_CANDIDATES = 4096;  // candidate_capacity at most: the kept list of the sift sits in LDS, as k_circle_sift's
constexpr int FEAT_PASSES = 3;
constexpr int FEAT_BINS = 2048;
constexpr int FEAT_GROUP_ROWS = 32;
constexpr int FEAT_TRIP_PX = 62;
constexpr int FEAT_STATE_WORDS = 8;
// the words of a frame's state: the largest key of the frame; the cut key T (built digit by digit); how many candidates are
// still to admit among those that agree with T so far (after the last pass: the ties admitted); 1: the frame has no more
// candidates than the capacity, all are admitted; candidates with key > T; candidates admitted; corners kept
enum { FEAT_MAXKEY = 0, FEAT_T = 1, FEAT_NEED = 2, FEAT_ALL = 3, FEAT_NGT = 4, FEAT_NCAND = 5, FEAT_NKEPT = 6 };
HC_HOST_DEVICE inline u32 feat_key(u32 bits) { return ((int32_t)bits > 0 && bits <= 0x7F800000u) ? bits : 0u; }
HC_HOST_DEVICE inline int feat_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }  // digits of 11, 11 and 10 bits
HC_HOST_DEVICE inline u32 feat_digit(u32 key, int pass) { return pass == 0 ? key >> 21 : pass == 1 ? (key >> 10) & 0x7FFu : key & 0x3FFu; }
// the bits of a key above the digit of `pass`: what the earlier passes fixed
HC_HOST_DEVICE inline u32 feat_prefix(u32 key, int pass) { return pass == 0 ? 0u : pass == 1 ? key >> 21 : key >> 10; }
inline int feat_groups(int H) { return (H + FEAT_GROUP_ROWS - 1) / FEAT_GROUP_ROWS; }
struct FeatParams {
  const uint8_t *plane;    // float32 planes of W x H, 4-byte aligned
  size_t pitch, frame_stride;
  int W, H, nframes, ngroups;
  float quality;           // (float)quality_level
  long long min_d2;
  int candidate_capacity;  // 1 .. FEAT_MAX_CANDIDATES
  size_t corner_capacity;
  u32 *counts;             // [nframes]
  float *corners;          // [nframes][corner_capacity][2], or null with corner_capacity 0
  float *quality_out;      // [nframes][corner_capacity], or null
  // scratch, per frame of the pass
  int32_t *ranked, *kept;  // [candidate_capacity] int4 (key, x, y, 0): in the order of the cut / after the sift
  u32 *cand;               // [candidate_capacity] (key, index)
  u32 *hist;               // [FEAT_BINS]
  u32 *state;              // [FEAT_STATE_WORDS]
  u32 *rows;               // [H][2]: candidates with key > T / == T of the row, then their exclusive prefix sums
};

// k_pyr_down8 (flow.hip): cv::pyrDown of one-channel u8 planes (hc_pyr_down_device, where the arithmetic is stated).  The lane
// layout of k_gauss8 on the SOURCE plane: a wave owns a strip of PYR_STRIP_W source columns, lane l the 4 source pixels at
// strip * PYR_STRIP_W - 4 + 4 l, which are the 2 destination pixels at half that column; lanes 0 and 63 are halo.  A work item is
// (frame, strip, PYR_CHUNK_ROWS destination rows) with a warm-up of 3 source rows.
constexpr int PYR_STRIP_W = 248;     // source columns per wave: 124 destination columns
static_assert(PYR_STRIP_W == STRIP_W && PYR_STRIP_W % 4 == 0, "k_pyr_down8 uses the lane layout of k_gauss8; a lane's source group starts at an even destination column");
constexpr int PYR_CHUNK_ROWS = 32;   // destination rows per work item
constexpr int PYR_MIN_SIDE = 3;      // one reflection suffices
inline int pyr_half(int n) { return (n + 1) / 2; }
inline int pyr_strips(int W) { return (W + PYR_STRIP_W - 1) / PYR_STRIP_W; }
inline int pyr_chunks(int dH) { return (dH + PYR_CHUNK_ROWS - 1) / PYR_CHUNK_ROWS; }
struct PyrParams {
  const uint8_t *in;       // u8 planes of W x H; any alignment (in_aligned: base, pitch and frame stride are multiples of 4)
  size_t in_pitch, in_frame_stride;
  uint8_t *out;            // u8 planes of dW x dH; any alignment (out_aligned: base, pitch and frame stride are even)
  size_t out_pitch, out_frame_stride;
  int W, H, dW, dH, nframes;
  int in_aligned, out_aligned;
  int nstrips, nchunks, total_items;  // total_items = nframes * nstrips * nchunks
};

// k_lk_flow (flow.hip): one pyramid level of cv::calcOpticalFlowPyrLK (hc_lk_flow_device, where the arithmetic is stated).  One
// wave per (frame, point slot), 4 waves a workgroup; window pixel t = lane + 64 r (r < rounds) is (t % win, t / win).
constexpr int FLOW_MIN_WIN = 5, FLOW_MAX_WIN = 31, FLOW_MAX_ITERATIONS = 64, FLOW_MAX_LEVEL = 15;
constexpr int FLOW_WAVES = 4;  // waves (points) per workgroup
inline bool flow_win_ok(int win) { return win >= FLOW_MIN_WIN && win <= FLOW_MAX_WIN && (win & 1); }
// rounds of 64 window pixels, and the class the kernel is compiled for: the smallest of 1, 2, 4, 7, 10, 16 that holds them
inline int flow_rounds(int win) { return (win * win + 63) / 64; }
inline int flow_round_class(int win)
{
  const int r = flow_rounds(win);
  return r <= 1 ? 1 : r <= 2 ? 2 : r <= 4 ? 4 : r <= 7 ? 7 : r <= 10 ? 10 : 16;
}
struct FlowParams {
  const uint8_t *prev, *next;  // u8 planes of W x H with a common pitch and frame stride; any alignment
  size_t pitch, frame_stride;
  int W, H, level, nframes;
  const u32 *counts;           // [nframes]
  const float *prev_pts;       // [nframes][capacity][2], level-0 units
  float *next_pts;             // likewise, in / out
  size_t capacity;
  int win, max_iterations, use_initial;
  float eps2, min_eig;         // (float)(epsilon * epsilon), (float)min_eig_threshold
  uint8_t *status;             // [nframes][capacity]; written at level 0 only
  float *err;                  // [nframes][capacity] or null; level 0 only
  u32 groups;                  // workgroups per frame: ceil(capacity / FLOW_WAVES)
};

// k_hist256 (stats.hip): 256-bin histograms of u8 frames, all channels pooled.  A work item is (frame, chunk of rows); a wave
// counts its rows into a wave-private LDS histogram and adds the non-zero bins to hist[frame] with global atomics.
constexpr int HIST_MAX_CHUNK_ROWS = 64, HIST_MIN_CHUNK_ROWS = 8;
// rows per work item: about 8192 items per launch (32 waves for each of the 256 CUs: 20 are resident, profiles/auto_thr) where
// the batch allows it, in chunks of 8 to 64 rows -- a chunk ends with up to 256 atomics per wave, which 8 rows of any width
// worth counting outweigh.  Chosen by that reasoning; the rule has not been swept (1024 frames of 1080p run at the 64-row cap:
// 17 items per frame, 0.96 ms, profiles/auto_thr/README.md)
inline int hist_chunk_rows(int H, int nframes)
{
  const long long rows = (long long)H * nframes;
  const long long want = (rows + 8191) / 8192;
  const int r = (int)(want < HIST_MIN_CHUNK_ROWS ? HIST_MIN_CHUNK_ROWS : want > HIST_MAX_CHUNK_ROWS ? HIST_MAX_CHUNK_ROWS : want);
  return r < H ? r : H;
}
struct HistParams {
  const uint8_t *in;       // u8 frames, any alignment of base, pitch and frame stride
  size_t in_pitch, in_frame_stride;
  u32 *hist;               // [nframes][256], zeroed before the launch
  int row_bytes;           // width * channels: no byte outside [row, row + row_bytes) is read
  int H, nframes;
  int chunk_rows, nchunks, total_items;  // hist_chunk_rows; ceil(H / chunk_rows); nframes * nchunks
};

// k_edge_count / k_edge_scan / k_edge_emit (edge_points.hip): the coordinates of the non-zero pixels of u8 maps in raster order
// (cv::findNonZero) and their number (cv::countNonZero).  A work item is (frame, chunk of rows) as for k_hist256, by the same
// rule (hist_chunk_rows): an item's cost is dominated by reading its rows, as there, and chunks of 8 rows and more keep the
// table of per-item counts small (8K frames at 8-row chunks: 540 per frame).
struct EdgePointsParams {
  const uint8_t *map;      // u8 maps of W x H, one channel, any alignment of base, pitch and frame stride
  size_t pitch, frame_stride;
  u32 *items;              // scratch [nframes][nchunks]: the items' counts (k_edge_count), then their offsets in the frame's list (k_edge_scan)
  u32 *counts;             // [nframes]: the full number of non-zero pixels of each frame
  int32_t *points;         // [nframes][capacity][2] = (x, y), 8-byte aligned; unused when capacity == 0
  size_t capacity;
  int W, H, nframes;       // no byte outside [row, row + W) is read
  int chunk_rows, nchunks, total_items;  // hist_chunk_rows; ceil(H / chunk_rows); nframes * nchunks
};

// k_hough_vote / k_hough_peaks / k_hough_scan / k_hough_rank (hough.hip): cv::HoughLines' standard transform from the point
// lists of k_edge_emit.  One block describes one pass: `nframes` frames whose accumulators, peak lists and per-row counts lie in
// the context's scratch together (plan_hough_lines, host_plan.h, cuts a batch into passes and moves the frame pointers on).
constexpr int HOUGH_LDS_BYTES = 160 * 1024;  // one workgroup's LDS on gfx950: the longest accumulator row k_hough_vote can hold
constexpr int HOUGH_MAX_ROWS = 8;            // angles (accumulator rows) per workgroup of k_hough_vote, at most
constexpr int HOUGH_VOTE_THREADS = 512;
constexpr int HOUGH_RANK_THREADS = 256;      // peaks per workgroup of k_hough_rank, and per LDS tile of its comparison loop
constexpr int HOUGH_CUS = 256;               // the plan keeps k_hough_vote's grid at this many workgroups where the batch allows it
struct HoughParams {
  const int32_t *points;     // [nframes][point_capacity][2] = (x, y), 8-byte aligned: what k_edge_emit wrote
  const u32 *point_counts;   // [nframes]: frame f votes with its first min(count, point_capacity) points
  size_t point_capacity;
  const float *tab_cos, *tab_sin, *tab_theta;  // [numangle] each (hough_fill_tables), device memory of the context
  int32_t *accum;            // scratch [nframes][numangle + 2][numrho + 2]: written whole by k_hough_vote
  u32 *items;                // scratch [nframes][numangle]: peaks of each angle row (k_hough_peaks), then their offsets (k_hough_scan)
  u32 *peaks;                // scratch [nframes][peak_cap][2] = (votes, accumulator index) in index order
  u32 *line_counts;          // [nframes]: the full number of peaks of each frame
  float *lines;              // [nframes][line_capacity][3] = (rho, theta, votes); unused when line_capacity == 0
  size_t line_capacity, peak_cap;  // peak_cap = numangle * ceil(numrho / 2): no frame has more peaks
  int numangle, numrho, nframes;
  int rows, groups;          // angles per workgroup of k_hough_vote (1 .. HOUGH_MAX_ROWS, rows * (numrho + 2) * 4 <= HOUGH_LDS_BYTES); ceil(numangle / rows)
  int threshold;             // a peak has more votes than this (>= 0)
  float rho;                 // (float)rho of the call: a line's distance is (r - (numrho - 1) * 0.5f) * rho
};

// k_seg_count / k_seg_scan / k_seg_emit (hough_segments.hip): the lines of k_hough_rank walked over the edge maps and cut into
// segments by a largest gap and a smallest length (cv::cuda::HoughSegmentDetector's form).  A work item is (frame, line slot)
// and belongs to one wave; slots at or above min(line_counts[frame], line_capacity) do nothing.
struct SegParams {
  const uint8_t *map;        // u8 maps of W x H, one channel, any alignment of base, pitch and frame stride
  size_t pitch, frame_stride;
  const float *lines;        // [nframes][line_capacity][3] = (rho, theta, votes): what k_hough_rank wrote
  const u32 *line_counts;    // [nframes]: frame f walks its first min(count, line_capacity) lines
  size_t line_capacity;
  const float *tab_theta;    // [numangle] (hough_fill_tables): a line's angle index is the first entry equal to its theta, bit for bit
  const int32_t *tab_major;  // [numangle] (hough_walk_tables): 0: one sample per column, 1: one sample per row
  const float *tab_slope, *tab_scale;  // [numangle]: sample m = rint(t * slope + line_rho * scale)
  u32 *items;                // scratch [nframes][line_capacity]: kept segments of each line (k_seg_count), then their offsets (k_seg_scan)
  u32 *seg_counts;           // [nframes]: the full number of kept segments of each frame
  int32_t *segs;             // [nframes][seg_capacity][4] = (x0, y0, x1, y1), 16-byte aligned; unused when seg_capacity == 0
  size_t seg_capacity;
  int W, H, nframes, numangle;  // no byte outside [row, row + W) is read
  int min_length, max_gap;   // both >= 0
  int total_items;           // nframes * line_capacity
};

// k_circle_vote / k_hough_peaks / k_hough_scan / k_circle_rank / k_circle_sift / k_circle_radii / k_circle_scan
// (hough_circles.hip): gradient-voted circle centres and per-centre radius histograms from the point lists of k_edge_emit and the
// int16 planes of k_deriv16 (cv::cuda::HoughCirclesDetector's form).  One block describes one pass, as HoughParams does.
constexpr int CIRCLE_MAX_CENTRES = 4096;     // centre_capacity at most: k_circle_sift keeps the kept list in LDS, 8 bytes a centre
constexpr int CIRCLE_MAX_HIST = 4096;        // words of a radius histogram (max_radius - min_radius + 3) at most: one workgroup's LDS table
constexpr int CIRCLE_THREADS = 256;          // points per workgroup trip of k_circle_vote and k_circle_radii
constexpr int CIRCLE_VOTE_GROUPS = 256;      // workgroups of k_circle_vote per frame at most: each strides over the frame's list
struct CircleParams {
  const int32_t *points;     // [nframes][point_capacity][2] = (x, y), 8-byte aligned: what k_edge_emit wrote
  const u32 *point_counts;   // [nframes]: frame f uses its first min(count, point_capacity) points
  size_t point_capacity;
  const int16_t *dx, *dy;    // int16 planes of W x H, one channel; pitch and frame_stride in BYTES, both even (H * pitch < 2^32)
  size_t pitch, frame_stride;
  int32_t *accum;            // scratch [nframes][AH + 2][AW + 2]: zeroed before k_circle_vote
  u32 *row_items;            // scratch [nframes][AH]: peaks of each accumulator row (k_hough_peaks), then their offsets (k_hough_scan)
  u32 *peaks;                // scratch [nframes][peak_cap][2] = (votes, accumulator index) in index order
  u32 *npeaks;               // scratch [nframes]: the peaks of each frame
  int32_t *ranked;           // scratch [nframes][centre_capacity][4] = (votes, cx, cy, 0): the first min(npeaks, centre_capacity) centres in order
  int32_t *kept;             // scratch [nframes][centre_capacity][4]: those of them the smallest distance keeps, in order
  u32 *nkept;                // scratch [nframes]
  u32 *items;                // scratch [nframes][centre_capacity]: circles of each kept centre (k_circle_radii<false>), then their offsets
  u32 *circle_counts;        // [nframes]: the full number of circles of each frame
  float *circles;            // [nframes][circle_capacity][4] = (x, y, radius, votes), 16-byte aligned; unused when circle_capacity == 0
  size_t circle_capacity, peak_cap;  // peak_cap = AH * ceil(AW / 2): no frame has more peaks
  long long min_d2;          // two kept centres are at least this far apart, squared, in accumulator cells
  int W, H, AW, AH, nframes;
  int centre_capacity;       // 1 .. CIRCLE_MAX_CENTRES
  int threshold;             // a centre has more votes than this, a circle at least this many (>= 0)
  int min_radius, max_radius;  // 1 <= min_radius <= max_radius, max_radius - min_radius + 3 <= CIRCLE_MAX_HIST
  float idp, dp;             // 1.0f / (float)dp and (float)dp of the call
  unsigned vote_groups;      // workgroups of k_circle_vote per frame (1 .. CIRCLE_VOTE_GROUPS)
  unsigned rank_groups;      // workgroups of k_circle_rank per frame: ceil(peak_cap / HOUGH_RANK_THREADS)
};

// k_ccl_local / k_ccl_merge / k_ccl_flatten / k_ccl_scan / k_ccl_roots / k_ccl_number / k_ccl_rows / k_ccl_stats / k_ccl_finish
// (ccl.hip): the connected components of u8 maps -- labels, number, and per component bounding box, area and centroid
// (cv::connectedComponentsWithStats).  The only per-pixel storage is the caller's label plane.  While the kernels run, a
// foreground pixel's label is 1 + the WORD index of a pixel of its component that lies before it in raster order, the word index
// of pixel (x, y) being y * (label_pitch / 4) + x: its place in the frame's label plane, which orders pixels as y * W + x does
// and needs no division to become an address (H * label_pitch < 2^32: below 2^30).  One block describes one pass, as
// HoughParams does: `nframes` frames whose per-chunk root counts lie in the context's table together.
constexpr int CCL_TILE_W = 64, CCL_TILE_H = 32;  // a workgroup of k_ccl_local: a row of the tile is one wave's ballot, 8 KiB of LDS labels
constexpr int CCL_THREADS = 256;
constexpr unsigned CCL_ROW_GROUPS = 1024;        // workgroups per frame of k_ccl_rows / k_ccl_finish at most: each strides over the rows
struct CclParams {
  const uint8_t *map;      // u8 maps of W x H, one channel, any alignment of base, pitch and frame stride
  size_t pitch, frame_stride;
  int32_t *labels;         // int32 [H][W] per frame; label_pitch and label_frame_stride in BYTES, multiples of 4, H * label_pitch < 2^32
  size_t label_pitch, label_frame_stride;
  u32 *items;              // scratch [nframes][nchunks]: the roots of a chunk of rows (k_ccl_flatten), then the roots before it (k_ccl_scan)
  u32 *counts;             // [nframes]: components + 1
  int32_t *stats;          // [nframes][capacity][5], 4-byte aligned; unused when capacity == 0
  unsigned long long *sums;  // the centroids [nframes][capacity][2], 8-byte aligned: the int64 sums of x and y until k_ccl_finish divides them
  size_t capacity;
  int W, H, nframes;
  int connectivity;        // 4 or 8
  int tiles_x, tiles_y;    // ceil(W / CCL_TILE_W), ceil(H / CCL_TILE_H)
  unsigned border_items;   // per frame: (tiles_y - 1) * W pixels below a horizontal tile border + (tiles_x - 1) * H right of a vertical one
  int chunk_rows, nchunks, total_items;  // hist_chunk_rows of the call; ceil(H / chunk_rows); nframes * nchunks
  unsigned row_groups;     // workgroups per frame of k_ccl_rows / k_ccl_finish: ceil(min(capacity, W * H + 1) / CCL_THREADS), at most CCL_ROW_GROUPS
};

// k_dt_cols / k_dt_rows (dist.hip): the exact squared Euclidean distance of every pixel of u8 maps to the nearest feature pixel,
// and that pixel (hc_distance_transform_device, where the result is stated).  The only per-pixel storage is the caller's distance
// plane: between the two kernels word (x, y) holds dy = y' - y of the nearest feature pixel (x, y') of column x, a tie between
// above and below going to the one above, or DT_NO_DY in a column without one.  |dy| <= H - 1 < DT_NO_DY, and nothing squares or
// compares DT_NO_DY: a word that holds it is skipped.
constexpr int DT_COL_THREADS = 64;   // a workgroup of k_dt_cols: one wave, one column per lane (a small batch spreads over more CUs)
constexpr int DT_COLS_PER_LANE = 1;  // as k_ccl_local: one byte, one word per lane whatever the views' alignment
constexpr int DT_LOOKAHEAD = 8;      // rows k_dt_cols loads before it walks them: the loads do not depend on the carried state
constexpr int DT_ROW_THREADS = 256;  // a workgroup of k_dt_rows: lane t owns the columns t, t + 256, ... of its row
constexpr int DT_ROWS = 4;           // rows a workgroup of k_dt_rows takes, one after the other, through the same LDS row
constexpr int DT_MAX_W = 16384;      // the LDS row of k_dt_rows: W int32, 64 KiB at most
constexpr int DT_NO_DY = 0x7FFFFFFF, DT_NONE = 0x7FFFFFFF;  // DT_NONE: HC_DT_NONE (host_plan.h asserts the match)
constexpr int DT_TO_NONZERO = 0, DT_TO_ZERO = 1, DT_SQUARED_I32 = 0, DT_F32 = 1;  // HC_DT_* (likewise)
struct DistParams {
  const uint8_t *map;      // u8 maps of W x H, one channel, any alignment of base, pitch and frame stride
  size_t pitch, frame_stride;
  int32_t *dist;           // int32 / float32 [H][W] per frame; pitch and frame stride in BYTES, multiples of 4, H * dist_pitch < 2^32
  size_t dist_pitch, dist_frame_stride;
  int32_t *nearest;        // int32 [H][W] per frame, likewise; null: not wanted
  size_t nearest_pitch, nearest_frame_stride;
  int W, H, nframes;       // (W - 1)^2 + (H - 1)^2 < 2^31 - 1, W * H < 2^31 - 1, W <= DT_MAX_W
  int target, dist_type;   // DT_TO_NONZERO / DT_TO_ZERO; DT_SQUARED_I32 / DT_F32
  unsigned col_groups;     // workgroups of k_dt_cols per frame: ceil(W / (DT_COL_THREADS * DT_COLS_PER_LANE))
  unsigned row_groups;     // workgroups of k_dt_rows per frame: ceil(H / DT_ROWS)
  unsigned lds_bytes;      // dynamic LDS of k_dt_rows: 4 * W
};

struct HystParams {
  u32 *sbits;
  const u32 *cbits;
  int RD, H, nframes;
  int tile_rows;   // rows per wave
  int waves;       // waves per workgroup; a workgroup tile is waves * tile_rows rows
  int nrtiles;     // row tiles per frame = ceil(H / (waves * tile_rows))
  int npanels;     // column panels per row tile = RD / 64 (a panel = 64 dwords = 2048 columns)
  u32 *flags;      // flags[k] != 0: launch k changed a tile-boundary row (another launch is needed)
  // How launches >= 1 find the tiles with work: a tile that changes a boundary row / column leaves a reason word with the
  // neighbours that look at it; wide frames also append them to the next launch's worklist.  [2] = launch parity;
  // wl_stride >= nframes * nrtiles * npanels words.
  u32 *wl_count;   // [launches + 1] wide frames: tiles on the list of (visited by) launch k; zero at the start of a run
  u32 *wl_reason;  // [2][wl_stride] per tile: 1 a tile above changed (its `top`), 2 below, 4 beside; zero at the start of a run
  u32 *wl_list;    // [2][wl_stride] wide frames: tile ids (frame * tiles per frame + tile)
  size_t wl_stride;
  int lists;       // this launch: 1 takes its tiles from the worklist; 0 a workgroup per tile; 2 a workgroup per tile that also writes the next launch's list (k_hyst's modes: hyst_mode, hyst.hip)
  int late_grid;   // worklist scheme: workgroups of launches >= 1 (0 = by the tile count, launch_hyst)
  int iter;        // index of this launch
  u32 *stats;      // optional diagnostics (3 words per launch) or null
  // fused expand: every launch also writes the 0/255 u8 rows it owns (launch 0: all rows of the tile,
  // later launches: the rows they changed), so no separate bit-plane -> u8 pass is needed
  uint8_t *out;
  size_t out_pitch, out_frame_stride;
  int W;
  int prov;        // the output already holds 255 for every strong pixel of the input planes (written by k_nms): launch 0 only rewrites rows it changes
  int first_pass;  // the planes come straight from k_front / k_pack: rows are not yet closed under the in-row fill
};

struct PackParams {  // tri-state u8 map (0/128/255) -> bit planes
  const uint8_t *in;
  size_t in_pitch, in_frame_stride;
  u32 *sbits, *cbits;
  int RD, W, H, nframes;
};

// ---- work split of the front kernels ----------------------------------------------------------
// front8.hip: 8 px per lane
constexpr int F8_STRIP_W = 62 * 8;   // 496 output columns per wave
constexpr int F8_HSTRIP_W = 30 * 8;  // HALF form: 240 output columns per half-wave (lanes 0 / 31 and 32 / 63 are its halo lanes)
constexpr int F8_SUB = 6;            // rows per window = lcm(2, 3) rows: the d / s register ring has period 2
inline int front8_run_rows(int windows) { return F8_SUB * windows - 4; }
inline int front8_strips(int W) { return (W + F8_STRIP_W - 1) / F8_STRIP_W; }
inline int front8_half_strips(int W) { return (W + F8_HSTRIP_W - 1) / F8_HSTRIP_W; }
// front_mx.hip
constexpr int MX_STRIP_W = 216;  // output columns per strip: 7 tiles of 28 + 20 columns of the eighth
constexpr int MX_ROWS = 16;      // rows per block
constexpr int MX_LAG = 4;        // the Sobel stage's rows trail the blur stage's by 4
inline int front_mx_strips(int W) { return (W + MX_STRIP_W - 1) / MX_STRIP_W; }
inline int front_mx_run_rows(int blocks) { return MX_ROWS * blocks - MX_LAG; }
// legacy_front.hip (the round-1 fused kernel)
constexpr int FSUB = 24;  // blur rows per sub-chunk: multiple of the prefetch group (4) and of the ring period (6)
inline int front_run_rows(int subchunks) { return FSUB * subchunks - 4; }

// ---- hysteresis workgroup shape ---------------------------------------------------------------
// k_hyst_loop (all rounds of a small run in one launch): at most this many tiles
constexpr int HYST_LOOP_MAX_TILES = 128;
// Workgroup tile = waves x tile_rows rows (hyst.hip).  The shapes k_hyst is compiled for, declared here once: the kernel
// launchers, the planner and its CPU test all go by this table.
struct HystShape { int tile_rows, waves; };
constexpr HystShape HYST_SHAPES[] = { { 32, 8 }, { 32, 4 }, { 32, 2 }, { 16, 8 }, { 32, 16 }, { 32, 1 }, { 16, 4 }, { 16, 2 } };
constexpr int N_HYST_SHAPES = (int)(sizeof(HYST_SHAPES) / sizeof(HYST_SHAPES[0]));
constexpr bool is_hyst_shape(int tile_rows, int waves)
{
  for (const HystShape &s : HYST_SHAPES)
    if (s.tile_rows == tile_rows && s.waves == waves) return true;
  return false;
}
// ... and the two that also have the looping kernel (k_hyst_loop)
constexpr bool hyst_shape_loops(int tile_rows, int waves) { return (tile_rows == 16 && waves == 8) || (tile_rows == 32 && waves == 2); }
static_assert(is_hyst_shape(16, 8) && is_hyst_shape(32, 2), "the looping shapes are shapes");
// Rounds of a tile's loop per launch (hyst_tile: between two rounds the waves of a workgroup exchange their boundary rows).  A
// path costs one round each time it passes from one wave's rows to another's; natural frames need a handful.  It is a budget,
// not a bound: content can need up to 2 * (waves - 1) * 2048 + 1 rounds (every round but the last sets a bit of a row another
// wave looks at) -- a 1-px path up and down the columns of a tile comes close -- and a tile that runs out of rounds flags the
// launch and leaves itself the reason that reopens its rows in the next one.  The budget keeps a launch short (4096 rounds are
// 27 ms of an 8-wave workgroup, 57 ms of a 16-wave one) for whoever waits for it: the other workgroups at k_hyst_loop's barrier, the next run's chain.
constexpr int HYST_ROUND_CAP = 4096;
// Patching a provisional map (hyst_tile's write-back): a changed row with at least this many changed 16-px groups is written
// whole, straight from its row register, instead of group by group through the LDS queue.  The queue suits the two or three
// groups a row of a camera-like frame changes; a row of dense content (iid noise: 87 of 120 groups at the median) costs it
// several LDS round trips and expansion passes of scattered stores.  The choice is per row and wave-uniform.
// (measured over 16 .. 64: DESIGN.md 3.3, profiles/r16_dense_rows)
#ifndef HC_HYST_ROW_FULL
#define HC_HYST_ROW_FULL 32  // (-D: the sweep's builds)
#endif
constexpr int HYST_ROW_FULL = HC_HYST_ROW_FULL;
static_assert(HYST_ROW_FULL >= 1 && HYST_ROW_FULL <= 128, "a panel row has 128 groups");
// 8 waves x 32 rows (256-row tiles) when the hysteresis has the chip to itself: fewer tile boundaries, fewer
// launches.  4 waves x 32 rows (one wave per SIMD) when it runs beside the next run's front kernels (pipelined mode):
// a 4-wave workgroup finds a place as soon as one wave slot per SIMD frees up, an 8-wave one has to wait for two --
// measured 1.7 ms against 4.2 ms for the hysteresis of 1024 frames under overlap.
// (beside k_front8, whose three workgroups fill a CU's LDS and registers, a hysteresis workgroup only finds room when a
// front workgroup retires: 2-wave workgroups fit the freed wave slots best -- 376 k frames/s against 368 k with 4 waves,
// 350 k with 8; one-wave workgroups need more launches than are queued for a 1080-row frame)
// frames_x_rows: frames x rows of the run.  geom: 0 = by the rules here; otherwise a shape of HYST_SHAPES picked by the caller for tuning experiments (encoded
// rows * 100 + waves, e.g. 3208 -- hc_create reads HC_HYST_GEOM once)
inline void hyst_tile_geometry(int geom, bool beside_front, long frames_x_rows, int H, int *tile_rows, int *waves)
{
  (void)H;
  *tile_rows = 32;
  *waves = beside_front ? 2 : 8;
  // (Taller frames had taller tiles here -- 4 waves above 1200 rows, 8 above 2400 -- from the time when 16 launches were
  // queued per run.  With up to 48 launches queued and the tile height following the content (plan_hyst), the small
  // 2-wave workgroups are as good at 4K (101 k frames/s either way) and better at 8K x 3 channels: 7.5 k against 6.6 k
  // frames/s -- an 8-wave workgroup needs two free wave slots on every SIMD of a CU at once, and launch 0 ran starved
  // beside the front kernel for as long as that took.)
  // a few frames only (the reference's one-frame-per-call pattern): the chip is nearly empty and the launches are pure
  // latency -- 8 waves x 16 rows per workgroup halve the rows a wave walks one after the other (measured on one 1080p
  // frame: hysteresis 0.122 ms against 0.139 ms with 8 x 32 and 0.130 ms with 4 x 32)
  if (frames_x_rows < 128 * 1024) { *tile_rows = 16; *waves = 8; }
  if (is_hyst_shape(geom / 100, geom % 100)) { *tile_rows = geom / 100; *waves = geom % 100; }
}

}  // namespace hc
