// The bodies csrc/keypoints.hip and csrc/keypoint_pyramid.hip share: one cell of the detection and one slot of the description
// (tests/keypoint_reference.py is the definition of both).  The single-scale kernels take the grey value from the colour image,
// the level kernels from a level's g8 plane; everything after that value is the same integer arithmetic.
#ifndef RTGS_KEYPOINT_COMMON_H
#define RTGS_KEYPOINT_COMMON_H
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

// the 8-bit grey value of a pixel inside the image, from the colour planes ...
struct GreyOfColor {
  const float* __restrict__ color;
  long long plane;
  __device__ __forceinline__ int operator()(long long at) const {
    const float grey = (0.299f * color[at] + 0.587f * color[plane + at]) + 0.114f * color[2 * plane + at];
    const float f = floorf(grey * 255.0f + 0.5f);
    return f >= 0.0f ? (f > 255.0f ? 255 : (int)f) : 0;            // a NaN is 0
  }
};

// ... or from a plane that holds it already
struct GreyOfPlane {
  const uint8_t* __restrict__ g8;
  __device__ __forceinline__ int operator()(long long at) const { return g8[at]; }
};

// One block of KP_THREADS threads, the cell (cx, cy) of c x c pixels of an H x W image: the cell's g8 with a halo of 4 is staged in
// LDS, out-of-image pixels as 0; box5 (and g8 where g8_out is given) of the cell's pixels go out, and slot[0 .. 3] = x, y, score,
// -1 of its keypoint, or 0, 0, 0, -1.  LDS: 40 x 40 B + 34 x 34 x 4 B + 16 B = 6 240 B.
template <class Grey>
__device__ __forceinline__ void detect_cell(const Grey grey, const float* __restrict__ depth, int H, int W, int c, int cx, int cy, int threshold,
                                            uint8_t* __restrict__ g8_out, int32_t* __restrict__ box_out, int32_t* __restrict__ slot) {
  __shared__ uint8_t g[(KP_MAXC + 2 * KP_HALO) * (KP_MAXC + 2 * KP_HALO)];
  __shared__ int sc[(KP_MAXC + 2) * (KP_MAXC + 2)];
  __shared__ unsigned wave_key[KP_WAVES];
  const int tid = threadIdx.x;
  const int x0 = cx * c, y0 = cy * c;
  const int tw = c + 2 * KP_HALO, sw = c + 2;
  for (int i = tid; i < tw * tw; i += KP_THREADS) {
    const int ty = i / tw, tx = i - ty * tw;
    const int x = x0 - KP_HALO + tx, y = y0 - KP_HALO + ty;
    int v = 0;
    if (x >= 0 && x < W && y >= 0 && y < H) v = grey((long long)y * W + x);
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
      if (g8_out) g8_out[at] = g[(ly + KP_HALO) * tw + lx + KP_HALO];
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
    if (key == 0) {
      slot[0] = 0;
      slot[1] = 0;
      slot[2] = 0;
    } else {
      const int i = 0xFFFF - (int)(key & 0xFFFFu);
      slot[0] = x0 + i % c;
      slot[1] = y0 + i / c;
      slot[2] = (int)(key >> 16);
    }
    slot[3] = -1;
  }
}

// One wave, one slot of an H x W image whose g8 and box5 planes are given: slot[3] = the orientation bin and desc[0 .. 7] = the
// descriptor; -1 and zeros for an empty slot (or one that is no slot of the detection).  Every lane of the wave calls it.
__device__ __forceinline__ void describe_slot(const uint8_t* __restrict__ g8, const int32_t* __restrict__ box, int H, int W, int oriented,
                                              const int32_t* __restrict__ dirs, const uint32_t* __restrict__ tables,
                                              int32_t* __restrict__ slot, uint32_t* __restrict__ desc, int lane) {
  const int x = slot[0], y = slot[1], s = slot[2];
  if (s <= 0 || x < KP_MARGIN || x >= W - KP_MARGIN || y < KP_MARGIN || y >= H - KP_MARGIN) {   // empty (or not a slot of detect)
    if (lane < 8) desc[lane] = 0u;
    if (lane == 0) slot[3] = -1;
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
      desc[2 * r] = (uint32_t)mask;
      desc[2 * r + 1] = (uint32_t)(mask >> 32);
    }
  }
  if (lane == 0) slot[3] = bin;
}

}  // namespace rtgs
#endif  // RTGS_KEYPOINT_COMMON_H
