// rtgs_keypoint_detect / rtgs_keypoint_describe / rtgs_keypoint_match (include/rtgs_slam.h): corners, binary descriptors and a
// brute-force Hamming match for the loop closure's wide-baseline revisits.  tests/keypoint_reference.py is the definition; after
// the grey value everything is integer arithmetic, so order does not matter and the kernels match it bit for bit.
//
// detect: one block of 256 threads per cell of c x c pixels (8 <= c <= 32).  The cell's g8 with a halo of 4 (1 for the 3 x 3
//   non-maximum suppression + 3 for the circle; box5's 2 lie within) is staged in LDS as bytes, out-of-image pixels as 0; from it
//   come the cell's g8 and box5 planes, then the eligible FAST-9 scores of the cell plus a halo of 1 (each computed once per cell,
//   into LDS), then the suppression and the cell's maximum as one packed key (score << 16 | 0xFFFF - row-major index in the cell):
//   a wave shuffle, then four keys through LDS.  LDS: 40 x 40 B + 34 x 34 x 4 B + 16 B = 6 240 B.
// describe: one wave per slot, four per block.  The two moments are int32 sums over the disc's 529 pixels (at most 13 x 255 x 529
//   < 2^31), reduced by butterflies; the 32 directions are scored in int64 by lanes 0 .. 31 and reduced with the tie rule; the
//   256 tests run as four rounds of 64, a ballot packs each round into two words.
// match: blockIdx.y is the (query set, reference set) pair, one wave per query, four queries per block; the block stages the
//   reference descriptors through LDS in tiles of 256 (8 KiB, word-major: lane l reads word w of reference j at [w][j], no bank
//   conflict), lane l takes references l, l + 64, ... of a tile, and the wave merges (best, index, second) by butterflies.
// No atomics, no host read; nothing here depends on the order in which blocks or waves run.  Compiled with -ffp-contract=off:
// the grey value's float32 chain is part of the definition.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/rtgs_slam.h"

namespace rtgs {

constexpr int KP_WAVE = 64;
constexpr int KP_WAVES = 4;
constexpr int KP_THREADS = KP_WAVE * KP_WAVES;
constexpr int KP_HALO = 4;
constexpr int KP_MAXC = RTGS_KEYPOINT_MAX_CELL;
constexpr int KP_MARGIN = RTGS_KEYPOINT_MARGIN;
constexpr int KP_RADIUS = 13;
constexpr int KP_TILE = 256;
constexpr int KP_NONE = 257;

// the circle of radius 3, clockwise from (0, -3): tests/keypoint_reference.CIRCLE
__device__ __forceinline__ int fast9_score(const uint8_t* __restrict__ t, int tw, int x, int y) {
  constexpr int DX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
  constexpr int DY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
  const int p = t[y * tw + x];
  int d[16], lo[16], hi[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) d[i] = (int)t[(y + DY[i]) * tw + (x + DX[i])] - p;
  // min and max over the 9 consecutive d[i .. i + 8]: windows of 2, 4, 8, then the ninth
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    lo[i] = min(d[i], d[(i + 1) & 15]);
    hi[i] = max(d[i], d[(i + 1) & 15]);
  }
  int lo4[16], hi4[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    lo4[i] = min(lo[i], lo[(i + 2) & 15]);
    hi4[i] = max(hi[i], hi[(i + 2) & 15]);
  }
  int bright = INT_MIN, dark = INT_MIN;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int lo9 = min(min(lo4[i], lo4[(i + 4) & 15]), d[(i + 8) & 15]);
    const int hi9 = max(max(hi4[i], hi4[(i + 4) & 15]), d[(i + 8) & 15]);
    bright = max(bright, lo9);
    dark = max(dark, -hi9);                                        // min over k of (p - c) = -(max over k of (c - p))
  }
  return max(bright, dark);
}

__global__ void __launch_bounds__(KP_THREADS) keypoint_detect_kernel(const float* __restrict__ color, const float* __restrict__ depth, int H, int W,
                                                                      int c, int ncx, int threshold, uint8_t* __restrict__ g8_out,
                                                                      int32_t* __restrict__ box_out, int32_t* __restrict__ slots) {
  __shared__ uint8_t g[(KP_MAXC + 2 * KP_HALO) * (KP_MAXC + 2 * KP_HALO)];
  __shared__ int sc[(KP_MAXC + 2) * (KP_MAXC + 2)];
  __shared__ unsigned wave_key[KP_WAVES];
  const int tid = threadIdx.x;
  const int x0 = (int)blockIdx.x * c, y0 = (int)blockIdx.y * c;
  const int tw = c + 2 * KP_HALO, sw = c + 2;
  const long long plane = (long long)H * W;
  for (int i = tid; i < tw * tw; i += KP_THREADS) {
    const int ty = i / tw, tx = i - ty * tw;
    const int x = x0 - KP_HALO + tx, y = y0 - KP_HALO + ty;
    int v = 0;
    if (x >= 0 && x < W && y >= 0 && y < H) {
      const long long at = (long long)y * W + x;
      const float grey = (0.299f * color[at] + 0.587f * color[plane + at]) + 0.114f * color[2 * plane + at];
      const float f = floorf(grey * 255.0f + 0.5f);
      v = f >= 0.0f ? (f > 255.0f ? 255 : (int)f) : 0;             // a NaN is 0
    }
    g[i] = (uint8_t)v;
  }
  __syncthreads();
  for (int i = tid; i < c * c; i += KP_THREADS) {
    const int ly = i / c, lx = i - ly * c;
    const int x = x0 + lx, y = y0 + ly;
    if (x < W && y < H) {
      const long long at = (long long)y * W + x;
      const uint8_t* q = g + (ly + KP_HALO - 2) * tw + (lx + KP_HALO - 2);
      int sum = 0;
#pragma unroll
      for (int dy = 0; dy < 5; ++dy)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) sum += q[dy * tw + dx];
      g8_out[at] = g[(ly + KP_HALO) * tw + lx + KP_HALO];
      box_out[at] = sum;
    }
  }
  for (int i = tid; i < sw * sw; i += KP_THREADS) {
    const int ly = i / sw, lx = i - ly * sw;
    const int x = x0 - 1 + lx, y = y0 - 1 + ly;
    int s = 0;
    if (x >= KP_MARGIN && x < W - KP_MARGIN && y >= KP_MARGIN && y < H - KP_MARGIN) {
      const float z = depth[(long long)y * W + x];
      if (z > 0.0f && z <= FLT_MAX) {
        const int f = fast9_score(g, tw, lx + KP_HALO - 1, ly + KP_HALO - 1);
        if (f > threshold) s = f;
      }
    }
    sc[i] = s;
  }
  __syncthreads();
  unsigned key = 0;
  for (int i = tid; i < c * c; i += KP_THREADS) {
    const int ly = i / c, lx = i - ly * c;
    if (x0 + lx < W && y0 + ly < H) {
      const int* q = sc + (ly + 1) * sw + (lx + 1);
      const int s = q[0];
      if (s > 0 && s > q[-sw - 1] && s > q[-sw] && s > q[-sw + 1] && s > q[-1] && s >= q[1] && s >= q[sw - 1] && s >= q[sw] &&
          s >= q[sw + 1]) {
        const unsigned k = ((unsigned)s << 16) | (unsigned)(0xFFFF - i);
        key = k > key ? k : key;
      }
    }
  }
  for (int o = KP_WAVE / 2; o >= 1; o >>= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)key, o, KP_WAVE);
    key = other > key ? other : key;
  }
  if ((tid & (KP_WAVE - 1)) == 0) wave_key[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < KP_WAVES; ++w) key = wave_key[w] > key ? wave_key[w] : key;
    int32_t* out = slots + 4 * ((long long)blockIdx.y * ncx + blockIdx.x);
    if (key == 0) {
      out[0] = 0;
      out[1] = 0;
      out[2] = 0;
    } else {
      const int i = 0xFFFF - (int)(key & 0xFFFFu);
      out[0] = x0 + i % c;
      out[1] = y0 + i / c;
      out[2] = (int)(key >> 16);
    }
    out[3] = -1;
  }
}

__global__ void __launch_bounds__(KP_THREADS) keypoint_describe_kernel(const uint8_t* __restrict__ g8, const int32_t* __restrict__ box, int H, int W,
                                                                        int ncells, int oriented, const int32_t* __restrict__ dirs,
                                                                        const uint32_t* __restrict__ tables, int32_t* __restrict__ slots,
                                                                        uint32_t* __restrict__ desc) {
  const int lane = threadIdx.x & (KP_WAVE - 1);
  const int slot = (int)blockIdx.x * KP_WAVES + (threadIdx.x >> 6);
  if (slot >= ncells) return;                                      // wave-uniform: the shuffles below see whole waves
  const int x = slots[4 * (long long)slot], y = slots[4 * (long long)slot + 1], s = slots[4 * (long long)slot + 2];
  if (s <= 0 || x < KP_MARGIN || x >= W - KP_MARGIN || y < KP_MARGIN || y >= H - KP_MARGIN) {   // empty (or not a slot of detect)
    if (lane < 8) desc[8 * (long long)slot + lane] = 0u;
    if (lane == 0) slots[4 * (long long)slot + 3] = -1;
    return;
  }
  int bin = 0;
  if (oriented) {
    constexpr int D = 2 * KP_RADIUS + 1;
    int m10 = 0, m01 = 0;
    for (int i = lane; i < D * D; i += KP_WAVE) {
      const int dy = i / D - KP_RADIUS, dx = i % D - KP_RADIUS;
      if (dx * dx + dy * dy <= KP_RADIUS * KP_RADIUS) {
        const int v = g8[(long long)(y + dy) * W + (x + dx)];
        m10 += dx * v;
        m01 += dy * v;
      }
    }
    for (int o = KP_WAVE / 2; o >= 1; o >>= 1) {
      m10 += __shfl_xor(m10, o, KP_WAVE);
      m01 += __shfl_xor(m01, o, KP_WAVE);
    }
    long long v = LLONG_MIN;
    int k = lane;
    if (lane < 32) v = (long long)dirs[2 * lane] * (long long)m10 + (long long)dirs[2 * lane + 1] * (long long)m01;
    for (int o = KP_WAVE / 2; o >= 1; o >>= 1) {
      const long long ov = __shfl_xor(v, o, KP_WAVE);
      const int ok = __shfl_xor(k, o, KP_WAVE);
      if (ov > v || (ov == v && ok < k)) {
        v = ov;
        k = ok;
      }
    }
    bin = k;
  }
  const uint32_t* __restrict__ tab = tables + 256 * bin;
  for (int r = 0; r < 4; ++r) {
    const uint32_t w = tab[r * KP_WAVE + lane];
    // a table of the host's keeps |x|, |y| <= 13; the clamps keep any other table's reads inside the image
    const int x1 = min(max(x + (int)(int8_t)(w & 0xFF), 0), W - 1), y1 = min(max(y + (int)(int8_t)((w >> 8) & 0xFF), 0), H - 1);
    const int x2 = min(max(x + (int)(int8_t)((w >> 16) & 0xFF), 0), W - 1), y2 = min(max(y + (int)(int8_t)(w >> 24), 0), H - 1);
    const bool bit = box[(long long)y1 * W + x1] < box[(long long)y2 * W + x2];
    const unsigned long long mask = __ballot(bit);
    if (lane == 0) {
      desc[8 * (long long)slot + 2 * r] = (uint32_t)mask;
      desc[8 * (long long)slot + 2 * r + 1] = (uint32_t)(mask >> 32);
    }
  }
  if (lane == 0) slots[4 * (long long)slot + 3] = bin;
}

__global__ void __launch_bounds__(KP_THREADS) keypoint_match_kernel(const uint32_t* __restrict__ desc, long long n_desc, const int32_t* __restrict__ pairs,
                                                                     long long n_out, int32_t* __restrict__ out) {
  __shared__ uint32_t tile[8][KP_TILE];
  const int tid = threadIdx.x, lane = tid & (KP_WAVE - 1), wave = tid >> 6;
  const int32_t* p = pairs + 5 * (long long)blockIdx.y;
  const long long qb = p[0], qn = p[1], rb = p[2], rn = p[3], ob = p[4];
  // block-uniform exits, before any barrier: a table that points outside the buffers is not followed
  if (qb < 0 || qn < 0 || rb < 0 || rn < 0 || ob < 0 || qb + qn > n_desc || rb + rn > n_desc || ob + qn > n_out) return;
  const long long q0 = (long long)blockIdx.x * KP_WAVES;
  if (q0 >= qn) return;
  const long long q = q0 + wave;
  const bool live = q < qn;
  uint32_t qd[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) qd[w] = live ? desc[8 * (qb + q) + w] : 0u;
  int best = KP_NONE, idx = INT_MAX, second = KP_NONE;
  for (long long t0 = 0; t0 < rn; t0 += KP_TILE) {
    __syncthreads();                                               // the tile before this one has been read by every wave
    if (t0 + tid < rn) {
      const uint4* src = reinterpret_cast<const uint4*>(desc + 8 * (rb + t0 + tid));
      const uint4 a = src[0], b = src[1];
      tile[0][tid] = a.x;
      tile[1][tid] = a.y;
      tile[2][tid] = a.z;
      tile[3][tid] = a.w;
      tile[4][tid] = b.x;
      tile[5][tid] = b.y;
      tile[6][tid] = b.z;
      tile[7][tid] = b.w;
    }
    __syncthreads();
    if (live) {
      const int n = (int)(rn - t0 < KP_TILE ? rn - t0 : KP_TILE);
      for (int j = lane; j < n; j += KP_WAVE) {                    // ascending indices per lane: a strict < keeps the lowest
        int d = 0;
#pragma unroll
        for (int w = 0; w < 8; ++w) d += __popc(qd[w] ^ tile[w][j]);
        if (d < best) {
          second = best;
          best = d;
          idx = (int)(t0 + j);
        } else if (d < second) {
          second = d;
        }
      }
    }
  }
  if (!live) return;                                               // wave-uniform
  for (int o = KP_WAVE / 2; o >= 1; o >>= 1) {                     // the two sides of every step hold disjoint reference sets
    const int ob_ = __shfl_xor(best, o, KP_WAVE), oi = __shfl_xor(idx, o, KP_WAVE), os = __shfl_xor(second, o, KP_WAVE);
    const bool other = ob_ < best || (ob_ == best && oi < idx);
    const int loser = other ? best : ob_;
    if (other) {
      best = ob_;
      idx = oi;
    }
    second = min(min(second, os), loser);
  }
  if (lane == 0) {
    int32_t* o3 = out + 3 * (ob + q);
    o3[0] = idx == INT_MAX ? -1 : idx;
    o3[1] = best;
    o3[2] = second;
  }
}

}  // namespace rtgs

extern "C" int rtgs_keypoint_detect(const float* color_chw, const float* depth, int32_t H, int32_t W, int32_t cell, int32_t threshold,
                                    uint8_t* g8, int32_t* box5, int32_t* slots, void* stream) {
  if (!color_chw || !depth || !g8 || !box5 || !slots) return -1;
  if (H < 1 || W < 1 || (int64_t)H * W >= 2147483648LL) return -1;
  if (cell < RTGS_KEYPOINT_MIN_CELL || cell > RTGS_KEYPOINT_MAX_CELL || threshold < 0 || threshold > 255) return -1;
  const int ncx = (W + cell - 1) / cell, ncy = (H + cell - 1) / cell;
  if (ncy > 65535) return -1;
  const dim3 grid((unsigned)ncx, (unsigned)ncy), block(rtgs::KP_THREADS);
  hipLaunchKernelGGL(rtgs::keypoint_detect_kernel, grid, block, 0, (hipStream_t)stream, color_chw, depth, (int)H, (int)W, (int)cell, ncx,
                     (int)threshold, g8, box5, slots);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int rtgs_keypoint_describe(const uint8_t* g8, const int32_t* box5, int32_t H, int32_t W, int32_t n_slots, int32_t oriented,
                                      const int32_t* dirs, const uint32_t* tables, int32_t* slots, uint32_t* desc, void* stream) {
  if (!g8 || !box5 || !dirs || !tables || !slots || !desc) return -1;
  if (H < 1 || W < 1 || (int64_t)H * W >= 2147483648LL || n_slots < 0) return -1;
  if (n_slots == 0) return 0;
  const dim3 grid((unsigned)((n_slots + rtgs::KP_WAVES - 1) / rtgs::KP_WAVES)), block(rtgs::KP_THREADS);
  hipLaunchKernelGGL(rtgs::keypoint_describe_kernel, grid, block, 0, (hipStream_t)stream, g8, box5, (int)H, (int)W, (int)n_slots,
                     (int)(oriented != 0), dirs, tables, slots, desc);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int rtgs_keypoint_match(const uint32_t* desc, int64_t n_desc, const int32_t* pairs, int32_t n_pairs, int32_t max_queries,
                                   int32_t* out, int64_t n_out, void* stream) {
  if (n_pairs < 0 || n_desc < 0 || n_out < 0 || max_queries < 0 || n_pairs > 65535) return -1;
  if (n_desc >= 2147483648LL || n_out >= 2147483648LL) return -1;
  if (n_pairs == 0 || max_queries == 0) return 0;
  if (!desc || !pairs || !out || ((uintptr_t)desc & 15u)) return -1;
  const dim3 grid((unsigned)((max_queries + rtgs::KP_WAVES - 1) / rtgs::KP_WAVES), (unsigned)n_pairs), block(rtgs::KP_THREADS);
  hipLaunchKernelGGL(rtgs::keypoint_match_kernel, grid, block, 0, (hipStream_t)stream, desc, (long long)n_desc, pairs, (long long)n_out,
                     out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
