// rtgs_place_describe / rtgs_place_scores (include/rtgs_slam.h): place recognition by appearance for the loop closure.  A keyframe
// becomes a thumbnail of tw x th cell means (grey value, depth, share of pixels with depth); two keyframes are compared by the
// zero-mean normalised cross-correlation of their grey thumbnails over a small horizontal shift, with the depth thumbnails as
// a second witness.  tests/place_reference.py is the definition and the kernels match it bit for bit.
//
// THE WAVE ORDER, the one summation order of this file: a wave of 64 lanes sums a flat list v[0 .. n - 1] in float64; lane l adds
// v[l], v[l + 64], ... in that order onto +0.0, then six butterfly steps o = 32 .. 1 replace every lane's value by its own plus
// that of lane l ^ o.  Float64 addition commutes bit for bit, so every lane ends with lane 0's value, the tree
// t[:o] = t[:o] + t[o:2o] of place_reference.wave_sum - and the whole wave can go on with it, no broadcast needed.  A missing
// or gated-out element is skipped: a sum that started at +0.0 never holds -0.0, so adding +0.0 would change nothing.
//
// describe: one wave per cell, four cells per block; the cell's flat list runs row by row, so a wave reads row segments of the
//   cell's width (120 B at 1200 x 680 -> 40 x 23, 32 B at 320 x 240 -> 40 x 30) next to each other.  3 x 4 B in, nothing kept.
// scores: one wave per pair, the four waves of a block share keyframe b.  The two grey thumbnails are loaded once into LDS
//   (b's once per block) and all 2 S + 1 shifts read them from there; the depth term runs once, at the chosen shift, and reads
//   the depth and valid thumbnails from memory (they are L2-resident: every a of a row reads the same b).  LDS: 5 thumbnails of
//   4 B cells, 24 000 B at 40 x 30.
// No atomics, no host read; the products of two float32 values are exact in float64, so the contraction of a b + acc is not
// part of the definition - the grey value's float32 chain is, and this file is compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rtgs_slam.h"

namespace rtgs {

constexpr int PLACE_WAVE = 64;
constexpr int PLACE_WAVES = 4;

__device__ __forceinline__ double place_wave_sum(double v) {
  for (int o = PLACE_WAVE / 2; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, PLACE_WAVE);
  return v;
}

__global__ void __launch_bounds__(PLACE_WAVE * PLACE_WAVES) place_describe_kernel(const float* __restrict__ color, const float* __restrict__ depth,
                                                                               int H, int W, int tw, int th, float* __restrict__ intensity_out,
                                                                               float* __restrict__ depth_out, float* __restrict__ valid_out) {
  const int lane = threadIdx.x & (PLACE_WAVE - 1);
  const int cell = blockIdx.x * PLACE_WAVES + (threadIdx.x >> 6);
  if (cell >= tw * th) return;                                   // wave-uniform: the shuffles below see whole waves
  const int ci = cell / tw, cj = cell - ci * tw;
  const int r0 = (int)(((long long)ci * H) / th), r1 = (int)(((long long)(ci + 1) * H) / th);
  const int c0 = (int)(((long long)cj * W) / tw), c1 = (int)(((long long)(cj + 1) * W) / tw);
  const int cw = c1 - c0, n = (r1 - r0) * cw;
  const long long plane = (long long)H * W;
  double sg = 0.0, sz = 0.0;
  int cnt = 0;
  int i = lane / cw, x = lane - i * cw;
  const int qi = PLACE_WAVE / cw, qx = PLACE_WAVE - qi * cw;
  for (int p = lane; p < n; p += PLACE_WAVE) {
    const long long at = (long long)(r0 + i) * W + (c0 + x);
    const float r = color[at], g = color[plane + at], b = color[2 * plane + at], z = depth[at];
    const float grey = (0.299f * r + 0.587f * g) + 0.114f * b;
    sg = sg + (double)grey;
    if (z > 0.0f) {
      sz = sz + (double)z;
      cnt++;
    }
    i += qi;
    x += qx;
    if (x >= cw) {
      x -= cw;
      i++;
    }
  }
  sg = place_wave_sum(sg);
  sz = place_wave_sum(sz);
  for (int o = PLACE_WAVE / 2; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, PLACE_WAVE);
  if (lane == 0) {
    intensity_out[cell] = (float)(sg / (double)n);
    depth_out[cell] = cnt > 0 ? (float)(sz / (double)cnt) : 0.0f;
    valid_out[cell] = (float)((double)cnt / (double)n);
  }
}

// the float64 score of one shift from the two grey thumbnails in LDS; every lane returns the same value
__device__ __forceinline__ double place_zncc(const float* __restrict__ A, const float* __restrict__ B, int tw, int th, int s, int lane) {
  const int x0 = s < 0 ? -s : 0, ow = tw - (s < 0 ? -s : s), n = th * ow;
  double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
  int i = lane / ow, x = lane - i * ow;
  const int qi = PLACE_WAVE / ow, qx = PLACE_WAVE - qi * ow;
  for (int p = lane; p < n; p += PLACE_WAVE) {
    const int at = i * tw + x0 + x;
    const double a = (double)A[at], b = (double)B[at + s];
    sa = sa + a;
    sb = sb + b;
    saa = saa + a * a;
    sbb = sbb + b * b;
    sab = sab + a * b;
    i += qi;
    x += qx;
    if (x >= ow) {
      x -= ow;
      i++;
    }
  }
  sa = place_wave_sum(sa);
  sb = place_wave_sum(sb);
  saa = place_wave_sum(saa);
  sbb = place_wave_sum(sbb);
  sab = place_wave_sum(sab);
  const double dn = (double)n;
  const double ma = sa / dn, mb = sb / dn;
  const double va = saa / dn - ma * ma, vb = sbb / dn - mb * mb, cov = sab / dn - ma * mb;
  if (va <= 1e-12 || vb <= 1e-12) return -1.0;
  return cov / sqrt(va * vb);
}

__global__ void __launch_bounds__(PLACE_WAVE * PLACE_WAVES) place_scores_kernel(const float* __restrict__ intensity, const float* __restrict__ depth,
                                                                             const float* __restrict__ valid, int M, int tw, int th, int S,
                                                                             int min_gap, int b_begin, float* __restrict__ score,
                                                                             int* __restrict__ shift, float* __restrict__ depth_rel) {
  extern __shared__ float place_lds[];                           // [cells] of b, then [cells] of a per wave
  const int cells = tw * th;
  const int lane = threadIdx.x & (PLACE_WAVE - 1), wave = threadIdx.x >> 6;
  const int b = b_begin + (int)blockIdx.x;
  const int a = (int)blockIdx.y * PLACE_WAVES + wave;
  const int n_a = b - min_gap + 1;                               // the a of this row that are computed: 0 .. n_a - 1
  if ((int)blockIdx.y * PLACE_WAVES >= n_a) {                    // a block of sentinels only (block-uniform: no barrier is skipped by some)
    if (a < M && lane == 0) {
      const long long at = (long long)b * M + a;
      score[at] = -2.0f;
      shift[at] = 0;
      depth_rel[at] = INFINITY;
    }
    return;
  }
  float* Bs = place_lds;
  float* As = place_lds + (size_t)cells * (1 + wave);
  const bool live = a < n_a;
  for (int c = threadIdx.x; c < cells; c += PLACE_WAVE * PLACE_WAVES) Bs[c] = intensity[(long long)b * cells + c];
  if (live)
    for (int c = lane; c < cells; c += PLACE_WAVE) As[c] = intensity[(long long)a * cells + c];
  __syncthreads();
  if (a >= M) return;
  const long long out = (long long)b * M + a;
  if (!live) {
    if (lane == 0) {
      score[out] = -2.0f;
      shift[out] = 0;
      depth_rel[out] = INFINITY;
    }
    return;
  }
  double best = place_zncc(As, Bs, tw, th, 0, lane);
  int best_s = 0;
  for (int k = 1; k <= S; ++k) {                                 // 0, -1, +1, -2, +2, ...: a later shift wins only if strictly greater
    const double zm = place_zncc(As, Bs, tw, th, -k, lane);
    if (zm > best) {
      best = zm;
      best_s = -k;
    }
    const double zp = place_zncc(As, Bs, tw, th, k, lane);
    if (zp > best) {
      best = zp;
      best_s = k;
    }
  }
  // the depth term at the chosen shift, over the same flat list
  const int s = best_s, x0 = s < 0 ? -s : 0, ow = tw - (s < 0 ? -s : s), n = th * ow;
  const float* __restrict__ Da = depth + (long long)a * cells;
  const float* __restrict__ Db = depth + (long long)b * cells;
  const float* __restrict__ Va = valid + (long long)a * cells;
  const float* __restrict__ Vb = valid + (long long)b * cells;
  double num = 0.0, den = 0.0;
  int cnt = 0;
  int i = lane / ow, x = lane - i * ow;
  const int qi = PLACE_WAVE / ow, qx = PLACE_WAVE - qi * ow;
  for (int p = lane; p < n; p += PLACE_WAVE) {
    const int at = i * tw + x0 + x;
    if (Va[at] >= 0.5f && Vb[at + s] >= 0.5f) {
      const double da = (double)Da[at], db = (double)Db[at + s];
      num = num + fabs(da - db);
      den = den + (da + db);
      cnt++;
    }
    i += qi;
    x += qx;
    if (x >= ow) {
      x -= ow;
      i++;
    }
  }
  num = place_wave_sum(num);
  den = place_wave_sum(den);
  for (int o = PLACE_WAVE / 2; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, PLACE_WAVE);
  if (lane == 0) {
    score[out] = (float)best;
    shift[out] = best_s;
    depth_rel[out] = 4 * cnt < n ? INFINITY : (float)(num / (0.5 * den));
  }
}

}  // namespace rtgs

extern "C" int rtgs_place_describe(const float* color_chw, const float* depth, int32_t H, int32_t W, int32_t tw, int32_t th,
                                   float* intensity_out, float* depth_out, float* valid_out, void* stream) {
  if (!color_chw || !depth || !intensity_out || !depth_out || !valid_out) return -1;
  if (H < 1 || W < 1 || (int64_t)H * W >= 2147483648LL || tw < 1 || th < 1 || tw > W || th > H) return -1;
  if ((int64_t)tw * th > RTGS_PLACE_MAX_CELLS) return -1;
  const int cells = tw * th;
  const dim3 grid((unsigned)((cells + rtgs::PLACE_WAVES - 1) / rtgs::PLACE_WAVES)), block(rtgs::PLACE_WAVE * rtgs::PLACE_WAVES);
  hipLaunchKernelGGL(rtgs::place_describe_kernel, grid, block, 0, (hipStream_t)stream, color_chw, depth, (int)H, (int)W, (int)tw, (int)th,
                     intensity_out, depth_out, valid_out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int rtgs_place_scores(const float* intensity, const float* depth, const float* valid, int32_t M, int32_t tw, int32_t th,
                                 int32_t S, int32_t min_gap, int32_t b_begin, int32_t b_end, float* score, int32_t* shift,
                                 float* depth_rel, void* stream) {
  if (!intensity || !depth || !valid || !score || !shift || !depth_rel) return -1;
  if (M < 1 || M > RTGS_PLACE_MAX_KEYFRAMES || tw < 1 || th < 1 || (int64_t)tw * th > RTGS_PLACE_MAX_CELLS) return -1;
  if (S < 0 || 2 * (int64_t)S >= tw || min_gap < 1 || b_begin < 0 || b_begin > b_end || b_end > M) return -1;
  if (b_begin == b_end) return 0;
  const int cells = tw * th;
  const dim3 grid((unsigned)(b_end - b_begin), (unsigned)((M + rtgs::PLACE_WAVES - 1) / rtgs::PLACE_WAVES)),
      block(rtgs::PLACE_WAVE * rtgs::PLACE_WAVES);
  const size_t lds = (size_t)cells * (1 + rtgs::PLACE_WAVES) * sizeof(float);
  hipLaunchKernelGGL(rtgs::place_scores_kernel, grid, block, lds, (hipStream_t)stream, intensity, depth, valid, (int)M, (int)tw, (int)th,
                     (int)S, (int)min_gap, (int)b_begin, score, shift, depth_rel);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
