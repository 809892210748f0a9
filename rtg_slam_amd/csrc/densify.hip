// gfx950 kernel + C ABI of the stable cloud's densification (include/rtgs_slam.h, "densification"): every stable Gaussian
// becomes K = sigma * levels * circle_num points on concentric ellipses around its mean, written as the records of
// save_model/pcd_densify.ply (x y z nx ny nz, float64).  Restates SLAM/gaussian_pointcloud.py:53-116 (densify) with the
// frame of get_normal / get_plane (:539-571) and build_rotation (utils/general_utils.py:108-132).
//
// Float chain (float32, one correctly rounded operation per step; built with -ffp-contract=off, Makefile EXTRA_densify):
//   q = rot / sqrt(((r r + x x) + y y) + z z), R = build_rotation(q)
//   axes: scales sorted ascending, ties to the lower index; n = column argmin of R, p0 / p1 = columns of the middle / largest
//         scale, each / (sqrt((c0 c0 + c1 c1) + c2 c2) + 1e-8); a0 / a1 = the middle / largest scale
//   point k = s (L C) + l C + c:  a = (a0 sigma) f32((l + 0.5) / L) + a0 s,  b likewise with a1,  x = a cos_c,  z = b sin_c,
//         offset = ((p0.x x + p0.y 0) + p0.z z, (n.x x + n.y 0) + n.z z, (p1.x x + p1.y 0) + p1.z z)   (the reference's M^T v)
//         point = offset + mu; its normal is n.
//
// Write-bound: 48 B per point.  A workgroup takes G Gaussians: G lanes build their frames into LDS, the workgroup builds the
// per-k table (cos, sin, level factor, ring) into LDS, then its G K 48 contiguous bytes are written as 16-B stores, lane i of
// a pass writing the i-th 16-B slot of the pass, so every wave store instruction covers 1 KB without a gap.  A slot is one of
// (x, y), (z, nx), (ny, nz) of a point; a lane computes the whole point and keeps two of its six values.
#include "../../include/rtgs_slam.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtgs_densify {

constexpr int NT = 256;
constexpr int G = 64;                 // Gaussians per workgroup
constexpr int FRAME = 16;             // floats of one Gaussian's frame in LDS
enum { MU = 0, NRM = 3, P0 = 6, P1 = 9, A0S = 12, A1S = 13, A0 = 14, A1 = 15 };

__device__ __forceinline__ void unit_column(const float R[3][3], int j, float* out) {
  const float c0 = R[0][j], c1 = R[1][j], c2 = R[2][j];
  const float d = sqrtf((c0 * c0 + c1 * c1) + c2 * c2) + 1e-8f;
  out[0] = c0 / d;
  out[1] = c1 / d;
  out[2] = c2 / d;
}

__global__ void __launch_bounds__(NT) densify_kernel(const float* __restrict__ xyz, const float* __restrict__ scales,
                                                     const float* __restrict__ rotations, int64_t row_begin, int64_t row_end,
                                                     const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                     int sigma, int levels, int circle_num, double* __restrict__ out) {
  extern __shared__ float4 lds[];
  const uint32_t K = (uint32_t)sigma * (uint32_t)levels * (uint32_t)circle_num;
  float4* tab = lds;                                               // [K]: cos_c, sin_c, f32((l + 0.5) / L), s
  float* frame = reinterpret_cast<float*>(lds + K);                // [G][FRAME]
  const int64_t g0 = row_begin + (int64_t)blockIdx.x * G;
  const int64_t left = row_end - g0;
  const uint32_t ng = left < G ? (uint32_t)left : (uint32_t)G;

  if (threadIdx.x < ng) {
    const int64_t row = g0 + threadIdx.x;
    float* f = frame + threadIdx.x * FRAME;
    const float s[3] = {scales[row * 3], scales[row * 3 + 1], scales[row * 3 + 2]};
    float r = rotations[row * 4], x = rotations[row * 4 + 1], y = rotations[row * 4 + 2], z = rotations[row * 4 + 3];
    const float qn = sqrtf(((r * r + x * x) + y * y) + z * z);
    r = r / qn; x = x / qn; y = y / qn; z = z / qn;
    const float R[3][3] = {{1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - r * z), 2.0f * (x * z + r * y)},
                           {2.0f * (x * y + r * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - r * x)},
                           {2.0f * (x * z - r * y), 2.0f * (y * z + r * x), 1.0f - 2.0f * (x * x + y * y)}};
    // stable ascending order of the three scales: i0 = argmin (first occurrence), then the other two, lower index first on a tie
    int i0 = s[1] < s[0] ? 1 : 0;
    if (s[2] < s[i0]) i0 = 2;
    const int j = i0 == 0 ? 1 : 0, k = i0 == 2 ? 1 : 2;
    const int i1 = s[k] < s[j] ? k : j, i2 = s[k] < s[j] ? j : k;
    f[MU] = xyz[row * 3]; f[MU + 1] = xyz[row * 3 + 1]; f[MU + 2] = xyz[row * 3 + 2];
    unit_column(R, i0, f + NRM);
    unit_column(R, i1, f + P0);
    unit_column(R, i2, f + P1);
    f[A0S] = s[i1] * (float)sigma;
    f[A1S] = s[i2] * (float)sigma;
    f[A0] = s[i1];
    f[A1] = s[i2];
  }
  const uint32_t LC = (uint32_t)levels * (uint32_t)circle_num;
  for (uint32_t k = threadIdx.x; k < K; k += NT) {
    const uint32_t ring = k / LC, rem = k - ring * LC, l = rem / (uint32_t)circle_num, c = rem - l * (uint32_t)circle_num;
    tab[k] = make_float4(cos_t[c], sin_t[c], (float)(((double)l + 0.5) / (double)levels), (float)ring);
  }
  __syncthreads();

  // slot t of the workgroup = (point t / 3, pair t % 3); the point = (Gaussian g, k); stepped by NT = 85 * 3 + 1 slots
  static_assert(NT % 3 == 1, "the slot stepping below assumes NT = 3 m + 1");
  const uint32_t n_slots = ng * K * 3;
  double* dst = out + (g0 - row_begin) * (int64_t)K * 6;
  uint32_t t = threadIdx.x;
  uint32_t pair = t % 3, pt = t / 3;
  uint32_t g = pt / K, k = pt - g * K;
  for (; t < n_slots; t += NT) {
    const float4 e = tab[k];
    const float* f = frame + g * FRAME;
    const float a = f[A0S] * e.z + f[A0] * e.w;
    const float b = f[A1S] * e.z + f[A1] * e.w;
    const float px = a * e.x, pz = b * e.y;
    const float ox = (f[P0] * px + f[P0 + 1] * 0.0f) + f[P0 + 2] * pz;
    const float oy = (f[NRM] * px + f[NRM + 1] * 0.0f) + f[NRM + 2] * pz;
    const float oz = (f[P1] * px + f[P1 + 1] * 0.0f) + f[P1 + 2] * pz;
    const float v[6] = {ox + f[MU], oy + f[MU + 1], oz + f[MU + 2], f[NRM], f[NRM + 1], f[NRM + 2]};
    const float lo = pair == 0 ? v[0] : (pair == 1 ? v[2] : v[4]);
    const float hi = pair == 0 ? v[1] : (pair == 1 ? v[3] : v[5]);
    *reinterpret_cast<double2*>(dst + 2 * (int64_t)t) = make_double2((double)lo, (double)hi);
    // advance by NT slots: 85 points and one pair
    uint32_t adv = NT / 3;
    if (++pair == 3) { pair = 0; ++adv; }
    k += adv;
    if (k >= K) { const uint32_t q = k / K; g += q; k -= q * K; }
  }
}

}  // namespace rtgs_densify

extern "C" {

int rtgs_densify_discs(const float* xyz, const float* scales, const float* rotations, int64_t row_begin, int64_t row_end,
                       const float* cos_theta, const float* sin_theta, int32_t sigma, int32_t levels, int32_t circle_num,
                       double* out, void* stream) {
  using namespace rtgs_densify;
  if (row_begin < 0 || row_end < row_begin || sigma <= 0 || levels <= 0 || circle_num <= 0) return -1;
  const int64_t K = (int64_t)sigma * levels * circle_num;
  if (K > RTGS_DENSIFY_MAX_POINTS_PER_GAUSSIAN) return -1;
  const int64_t P = row_end - row_begin;
  if (P == 0) return 0;
  if (!xyz || !scales || !rotations || !cos_theta || !sin_theta || !out || ((uintptr_t)out & 15u) != 0) return -1;
  const int64_t blocks = (P + G - 1) / G;
  if (blocks > 0x7fffffffLL) return -1;
  const size_t lds = (size_t)K * sizeof(float4) + (size_t)G * FRAME * sizeof(float);
  hipLaunchKernelGGL(densify_kernel, dim3((unsigned)blocks), dim3(NT), lds, (hipStream_t)stream, xyz, scales, rotations,
                     row_begin, row_end, cos_theta, sin_theta, (int)sigma, (int)levels, (int)circle_num, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
