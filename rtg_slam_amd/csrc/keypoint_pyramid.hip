// rtgs_keypoint_pyramid / rtgs_keypoint_detect_levels / rtgs_keypoint_describe_levels / rtgs_keypoint_votes (include/rtgs_slam.h):
// the keypoints of csrc/keypoints.hip over an image pyramid, so that a revisit from another distance still matches, and the count
// of filtered matches per keyframe pair, by which revisits are found.  tests/keypoint_pyramid_reference.py is the definition;
// after the grey value everything is integer arithmetic, so the kernels match it bit for bit.
//
// THE LADDER.  Scales 1, 3/2, 2, 3, 4: level 1 is level 0 reduced 3:2, level 2 level 0 reduced 2:1, level 3 level 1 reduced 2:1,
// level 4 level 2 reduced 2:1.  All levels of a frame lie in one g8 buffer and one depth buffer, level l at levels[l][0].
// pyramid: one block of 256 threads per 48 x 48 tile of level 0.  48 is a multiple of 12, so the tile's 32 x 32 pixels of level 1,
//   24 x 24 of level 2, 16 x 16 of level 3 and 12 x 12 of level 4 depend on nothing outside it: the tile's g8 is staged in LDS
//   once (from the colour), levels 1 and 2 are made from it and kept in LDS, levels 3 and 4 from those.  A level's pixel inside its
//   image only reads pixels inside the image of the level above it (the sizes round down), so no border rule is needed.  The
//   depth of a level is one pixel of level 0's, never an average.  LDS: 2 304 + 1 024 + 576 B.
// detect_levels, describe_levels: detect_cell and describe_slot of keypoint_common.h; blockIdx.x runs over the cells (the slots)
//   of all levels, level after level, and the level is found from the table's prefix of cells.
// votes: one wave per pair, four per block; 64 rows of the b-against-a table a round, a ballot and a population count.
// No atomics, no host read; nothing here depends on the order in which blocks or waves run.  Compiled with -ffp-contract=off:
// the grey value's float32 chain is part of the definition.
#include "keypoint_common.h"

namespace rtgs {

constexpr int KP_LEVELS = RTGS_KEYPOINT_MAX_LEVELS;
constexpr int KP_T0 = 48, KP_T1 = 32, KP_T2 = 24, KP_T3 = 16, KP_T4 = 12;

// the level table by value: first pixel, height, width and first cell (slot) of every level, cells[n] the total
struct KpLevels {
  int n;
  int off[KP_LEVELS];
  int H[KP_LEVELS];
  int W[KP_LEVELS];
  int ncx[KP_LEVELS];
  int cells[KP_LEVELS + 1];
};

__global__ void __launch_bounds__(KP_THREADS) keypoint_pyramid_kernel(const float* __restrict__ color, const float* __restrict__ depth, KpLevels lv,
                                                                       uint8_t* __restrict__ g8, float* __restrict__ dl) {
  __shared__ uint8_t t0[KP_T0 * KP_T0];
  __shared__ uint8_t t1[KP_T1 * KP_T1];
  __shared__ uint8_t t2[KP_T2 * KP_T2];
  const int tid = threadIdx.x;
  const int H = lv.H[0], W = lv.W[0];
  const int bx = (int)blockIdx.x, by = (int)blockIdx.y;
  const GreyOfColor grey{color, (long long)H * W};
  for (int i = tid; i < KP_T0 * KP_T0; i += KP_THREADS) {
    const int ty = i / KP_T0, tx = i - ty * KP_T0;
    const int x = bx * KP_T0 + tx, y = by * KP_T0 + ty;
    int v = 0;
    if (x < W && y < H) {
      const long long at = (long long)y * W + x;
      v = grey(at);
      g8[lv.off[0] + at] = (uint8_t)v;
      dl[lv.off[0] + at] = depth[at];
    }
    t0[i] = (uint8_t)v;
  }
  __syncthreads();
  if (lv.n > 1) {                                                  // 3:2: output 2k takes inputs 3k, 3k + 1 with weights 2, 1; 2k + 1 takes 3k + 1, 3k + 2 with 1, 2
    const int H1 = lv.H[1], W1 = lv.W[1];
    for (int i = tid; i < KP_T1 * KP_T1; i += KP_THREADS) {
      const int ty = i / KP_T1, tx = i - ty * KP_T1;
      const int ox = tx & 1, oy = ty & 1;
      const int sx = 3 * (tx >> 1) + ox, sy = 3 * (ty >> 1) + oy;  // the first of the two inputs, in the tile
      const int wx0 = 2 - ox, wx1 = 1 + ox, wy0 = 2 - oy, wy1 = 1 + oy;
      const uint8_t* q = t0 + sy * KP_T0 + sx;
      const int v = (wy0 * (wx0 * q[0] + wx1 * q[1]) + wy1 * (wx0 * q[KP_T0] + wx1 * q[KP_T0 + 1]) + 4) / 9;
      t1[i] = (uint8_t)v;
      const int x = bx * KP_T1 + tx, y = by * KP_T1 + ty;
      if (x < W1 && y < H1) {
        const long long at = lv.off[1] + (long long)y * W1 + x;
        g8[at] = (uint8_t)v;
        dl[at] = depth[(long long)(by * KP_T0 + sy + oy) * W + (bx * KP_T0 + sx + ox)];      // floor((2 x + 1) 3 / 4) = 3 k + 2 (x odd)
      }
    }
  }
  if (lv.n > 2) {                                                  // 2:1: (a + b + c + d + 2) >> 2
    const int H2 = lv.H[2], W2 = lv.W[2];
    for (int i = tid; i < KP_T2 * KP_T2; i += KP_THREADS) {
      const int ty = i / KP_T2, tx = i - ty * KP_T2;
      const uint8_t* q = t0 + 2 * ty * KP_T0 + 2 * tx;
      const int v = (q[0] + q[1] + q[KP_T0] + q[KP_T0 + 1] + 2) >> 2;
      t2[i] = (uint8_t)v;
      const int x = bx * KP_T2 + tx, y = by * KP_T2 + ty;
      if (x < W2 && y < H2) {
        const long long at = lv.off[2] + (long long)y * W2 + x;
        g8[at] = (uint8_t)v;
        dl[at] = depth[(long long)(by * KP_T0 + 2 * ty + 1) * W + (bx * KP_T0 + 2 * tx + 1)];
      }
    }
  }
  if (lv.n <= 3) return;                                           // block-uniform
  __syncthreads();
  {
    const int H3 = lv.H[3], W3 = lv.W[3];
    for (int i = tid; i < KP_T3 * KP_T3; i += KP_THREADS) {
      const int ty = i / KP_T3, tx = i - ty * KP_T3;
      const uint8_t* q = t1 + 2 * ty * KP_T1 + 2 * tx;
      const int v = (q[0] + q[1] + q[KP_T1] + q[KP_T1 + 1] + 2) >> 2;
      const int x = bx * KP_T3 + tx, y = by * KP_T3 + ty;
      if (x < W3 && y < H3) {
        const long long at = lv.off[3] + (long long)y * W3 + x;
        g8[at] = (uint8_t)v;
        dl[at] = depth[(long long)(by * KP_T0 + 3 * ty + 1) * W + (bx * KP_T0 + 3 * tx + 1)];
      }
    }
  }
  if (lv.n > 4) {
    const int H4 = lv.H[4], W4 = lv.W[4];
    for (int i = tid; i < KP_T4 * KP_T4; i += KP_THREADS) {
      const int ty = i / KP_T4, tx = i - ty * KP_T4;
      const uint8_t* q = t2 + 2 * ty * KP_T2 + 2 * tx;
      const int v = (q[0] + q[1] + q[KP_T2] + q[KP_T2 + 1] + 2) >> 2;
      const int x = bx * KP_T4 + tx, y = by * KP_T4 + ty;
      if (x < W4 && y < H4) {
        const long long at = lv.off[4] + (long long)y * W4 + x;
        g8[at] = (uint8_t)v;
        dl[at] = depth[(long long)(by * KP_T0 + 4 * ty + 2) * W + (bx * KP_T0 + 4 * tx + 2)];
      }
    }
  }
}

__device__ __forceinline__ int level_of(const KpLevels& lv, int cell) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < KP_LEVELS; ++k) l += (k < lv.n && cell >= lv.cells[k]) ? 1 : 0;
  return l;
}

__global__ void __launch_bounds__(KP_THREADS) keypoint_detect_levels_kernel(const uint8_t* __restrict__ g8, const float* __restrict__ dl, KpLevels lv, int c,
                                                                             int threshold, int32_t* __restrict__ box, int32_t* __restrict__ slots) {
  const int cell = (int)blockIdx.x;
  const int l = level_of(lv, cell);
  const int local = cell - lv.cells[l], ncx = lv.ncx[l];
  detect_cell(GreyOfPlane{g8 + lv.off[l]}, dl + lv.off[l], lv.H[l], lv.W[l], c, local % ncx, local / ncx, threshold, (uint8_t*)nullptr,
              box + lv.off[l], slots + 4 * (long long)cell);
}

__global__ void __launch_bounds__(KP_THREADS) keypoint_describe_levels_kernel(const uint8_t* __restrict__ g8, const int32_t* __restrict__ box, KpLevels lv,
                                                                               int oriented, const int32_t* __restrict__ dirs,
                                                                               const uint32_t* __restrict__ tables, int32_t* __restrict__ slots,
                                                                               uint32_t* __restrict__ desc) {
  const int lane = threadIdx.x & (KP_WAVE - 1);
  const int slot = (int)blockIdx.x * KP_WAVES + (threadIdx.x >> 6);
  if (slot >= lv.cells[lv.n]) return;                              // wave-uniform: the shuffles of describe_slot see whole waves
  const int l = level_of(lv, slot);
  describe_slot(g8 + lv.off[l], box + lv.off[l], lv.H[l], lv.W[l], oriented, dirs, tables, slots + 4 * (long long)slot,
                desc + 8 * (long long)slot, lane);
}

__global__ void __launch_bounds__(KP_THREADS) keypoint_votes_kernel(const int32_t* __restrict__ matches, long long n_matches, const int32_t* __restrict__ pairs,
                                                                     int n_pairs, int max_hamming, double ratio, int32_t* __restrict__ votes) {
  const int lane = threadIdx.x & (KP_WAVE - 1);
  const int pair = (int)blockIdx.x * KP_WAVES + (threadIdx.x >> 6);
  if (pair >= n_pairs) return;                                     // wave-uniform, as every exit below
  const int32_t* p = pairs + 4 * (long long)pair;
  const long long mb = p[0], nb = p[1], ma = p[2], na = p[3];
  if (mb < 0 || nb < 0 || ma < 0 || na < 0 || mb + nb > n_matches || ma + na > n_matches) return;   // not followed: votes keeps what it held
  int count = 0;
  for (long long i0 = 0; i0 < nb; i0 += KP_WAVE) {
    const long long i = i0 + lane;
    bool keep = false;
    if (i < nb) {
      const int32_t* m = matches + 3 * (mb + i);
      const int j = m[0], d = m[1], second = m[2];
      keep = j >= 0 && j < na && (long long)matches[3 * (ma + j)] == i && d <= max_hamming && (double)d <= ratio * (double)second;
    }
    count += __popcll(__ballot(keep));
  }
  if (lane == 0) votes[pair] = count;
}

// the public table [n][5] (first pixel, H, W, num, den) checked against the ladder and the buffers, and turned into KpLevels;
// cell 0: no cells wanted
static bool levels_from_table(const int32_t* levels, int n, int64_t n_pixels, int cell, KpLevels* out) {
  static const int NUM[KP_LEVELS] = {1, 3, 2, 3, 4}, DEN[KP_LEVELS] = {1, 2, 1, 1, 1};
  if (!levels || n < 1 || n > KP_LEVELS || n_pixels < 1 || n_pixels >= 2147483648LL) return false;
  KpLevels lv = {};
  lv.n = n;
  for (int l = 0; l < n; ++l) {
    const int32_t* t = levels + 5 * l;
    const int64_t off = t[0], H = t[1], W = t[2];
    if (t[3] != NUM[l] || t[4] != DEN[l] || off < 0 || H < 1 || W < 1 || off + H * W > n_pixels) return false;
    if (l == 1 && (H != 2 * (lv.H[0] / 3) || W != 2 * (lv.W[0] / 3))) return false;
    if (l >= 2 && (H != lv.H[l - 2] / 2 || W != lv.W[l - 2] / 2)) return false;        // 2 from 0, 3 from 1, 4 from 2
    for (int k = 0; k < l; ++k)                                    // two levels do not share a pixel
      if (off < (int64_t)lv.off[k] + (int64_t)lv.H[k] * lv.W[k] && (int64_t)lv.off[k] < off + H * W) return false;
    lv.off[l] = (int)off;
    lv.H[l] = (int)H;
    lv.W[l] = (int)W;
    if (cell > 0) {
      const int64_t ncx = (W + cell - 1) / cell, ncy = (H + cell - 1) / cell;
      if ((int64_t)lv.cells[l] + ncx * ncy >= 2147483648LL) return false;
      lv.ncx[l] = (int)ncx;
      lv.cells[l + 1] = lv.cells[l] + (int)(ncx * ncy);
    }
  }
  for (int l = n; l < KP_LEVELS; ++l) lv.cells[l + 1] = lv.cells[n];
  *out = lv;
  return true;
}

}  // namespace rtgs

extern "C" int rtgs_keypoint_pyramid(const float* color_chw, const float* depth, const int32_t* levels, int32_t n_levels, int64_t n_pixels,
                                     uint8_t* g8, float* depth_levels, void* stream) {
  rtgs::KpLevels lv;
  if (!color_chw || !depth || !g8 || !depth_levels || !rtgs::levels_from_table(levels, n_levels, n_pixels, 0, &lv)) return -1;
  const int gx = (lv.W[0] + rtgs::KP_T0 - 1) / rtgs::KP_T0, gy = (lv.H[0] + rtgs::KP_T0 - 1) / rtgs::KP_T0;
  if (gy > 65535) return -1;
  const dim3 grid((unsigned)gx, (unsigned)gy), block(rtgs::KP_THREADS);
  hipLaunchKernelGGL(rtgs::keypoint_pyramid_kernel, grid, block, 0, (hipStream_t)stream, color_chw, depth, lv, g8, depth_levels);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int rtgs_keypoint_detect_levels(const uint8_t* g8, const float* depth_levels, const int32_t* levels, int32_t n_levels, int64_t n_pixels,
                                           int32_t cell, int32_t threshold, int32_t* box5, int32_t* slots, void* stream) {
  rtgs::KpLevels lv;
  if (!g8 || !depth_levels || !box5 || !slots) return -1;
  if (cell < RTGS_KEYPOINT_MIN_CELL || cell > RTGS_KEYPOINT_MAX_CELL || threshold < 0 || threshold > 255) return -1;
  if (!rtgs::levels_from_table(levels, n_levels, n_pixels, cell, &lv)) return -1;
  const dim3 grid((unsigned)lv.cells[lv.n]), block(rtgs::KP_THREADS);
  hipLaunchKernelGGL(rtgs::keypoint_detect_levels_kernel, grid, block, 0, (hipStream_t)stream, g8, depth_levels, lv, (int)cell, (int)threshold, box5,
                     slots);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int rtgs_keypoint_describe_levels(const uint8_t* g8, const int32_t* box5, const int32_t* levels, int32_t n_levels, int64_t n_pixels,
                                             int32_t cell, int32_t oriented, const int32_t* dirs, const uint32_t* tables, int32_t* slots,
                                             uint32_t* desc, void* stream) {
  rtgs::KpLevels lv;
  if (!g8 || !box5 || !dirs || !tables || !slots || !desc) return -1;
  if (cell < RTGS_KEYPOINT_MIN_CELL || cell > RTGS_KEYPOINT_MAX_CELL) return -1;
  if (!rtgs::levels_from_table(levels, n_levels, n_pixels, cell, &lv)) return -1;
  const dim3 grid((unsigned)((lv.cells[lv.n] + rtgs::KP_WAVES - 1) / rtgs::KP_WAVES)), block(rtgs::KP_THREADS);
  hipLaunchKernelGGL(rtgs::keypoint_describe_levels_kernel, grid, block, 0, (hipStream_t)stream, g8, box5, lv, (int)(oriented != 0), dirs, tables,
                     slots, desc);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int rtgs_keypoint_votes(const int32_t* matches, int64_t n_matches, const int32_t* pairs, int32_t n_pairs, int32_t max_hamming,
                                   double ratio, int32_t* votes, void* stream) {
  if (n_pairs < 0 || n_matches < 0 || n_matches >= 2147483648LL || !(ratio >= 0.0)) return -1;
  if (n_pairs == 0) return 0;
  if (!pairs || !votes || (n_matches > 0 && !matches)) return -1;
  const dim3 grid((unsigned)((n_pairs + rtgs::KP_WAVES - 1) / rtgs::KP_WAVES)), block(rtgs::KP_THREADS);
  hipLaunchKernelGGL(rtgs::keypoint_votes_kernel, grid, block, 0, (hipStream_t)stream, matches, (long long)n_matches, pairs, (int)n_pairs,
                     (int)max_hamming, ratio, votes);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
