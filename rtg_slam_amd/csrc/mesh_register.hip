// gfx950 kernels + C ABI of the mesh registration (include/rtgs_slam.h, "mesh registration"): the point-to-plane normal equations
// of N points against the faces rtgs_mesh_distance_query gave them - 21 + 6 + 3 float64 sums - in an order that depends on N alone.
// No counterpart in the reference; tests/mesh_register_reference.py restates the gates, the per-point terms and the order of
// summation in numpy and is the definition, matched bit for bit.  Built with -ffp-contract=off (Makefile EXTRA_mesh_register):
// every float32 and float64 step below is one correctly rounded operation.
//
// Two launches on the caller's stream:
// chunks     one workgroup of 256 threads per chunk of 1024 points.  Thread s is slot s: it adds the terms of the points
//            1024 chunk + s + 256 k, k = 0..3, that take part to 30 float64 registers that start at +0 (a sum that starts at +0
//            is never -0, so a point that does not take part may be skipped: adding its +0 would change no bit).  Then the
//            tree: six __shfl_down steps inside each wave, the four wave values through LDS, (w0 + w1) + (w2 + w3) by the first
//            30 threads, which store the chunk's 30 values to the scratch.
// total      one workgroup: slot s adds the chunk values s, s + 256, ... in order, the same tree, out[30].
// This is a streaming pass: 12 B of point, 4 B of face, 4 B of d2 (12 B of source normal) per point and three gathered corners;
// 720 float64 shuffles per wave and chunk are the arithmetic that is not per point.
//
// Index range: face[i] is tested against F; the caller guarantees 0 <= faces[.] < V (mesh_ops.MeshDistance checked it).
#include "../../include/rtgs_slam.h"
#include "mesh_face_normal.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace rtgs_mesh_register_k {

constexpr int NT = 256;
constexpr int WAVE = 64;
constexpr int WAVES = NT / WAVE;
constexpr int CHUNK = RTGS_MESH_REGISTER_CHUNK;
constexpr int OUT = RTGS_MESH_REGISTER_OUT;
static_assert(CHUNK % NT == 0 && WAVES == 4 && OUT <= NT, "the tree below is written for 4 waves of 64");

struct Center {
  float x, y, z;
};

// 256 slots -> one value per k, written to dst[k] by thread k.  Every thread of the workgroup calls it.
__device__ __forceinline__ void tree(double (&acc)[OUT], double* __restrict__ lds, double* __restrict__ dst) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < OUT; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = WAVE / 2; o >= 1; o >>= 1) v = v + __shfl_down(v, o, WAVE);      // lane 0 only ever reads lanes l + o < 2 o
    if (lane == 0) lds[wave * OUT + k] = v;
  }
  __syncthreads();
  if (threadIdx.x < OUT) {
    const int k = threadIdx.x;
    dst[k] = (lds[k] + lds[OUT + k]) + (lds[2 * OUT + k] + lds[3 * OUT + k]);
  }
}

__global__ void __launch_bounds__(NT) chunks_kernel(const float* __restrict__ points, const int32_t* __restrict__ face,
                                                    const float* __restrict__ d2, const float* __restrict__ src_normals, int64_t N,
                                                    const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t F,
                                                    Center c, float max_d2, float min_cos, double* __restrict__ partial) {
  __shared__ double lds[WAVES * OUT];
  double acc[OUT];
#pragma unroll
  for (int k = 0; k < OUT; ++k) acc[k] = 0.0;
  const int64_t base = (int64_t)blockIdx.x * CHUNK + threadIdx.x;
#pragma unroll 1
  for (int step = 0; step < CHUNK / NT; ++step) {
    const int64_t i = base + (int64_t)step * NT;
    if (i >= N) break;
    const int64_t f = face[i];
    if (f < 0 || f >= F) continue;
    const float dd = d2[i];
    if (!(dd <= max_d2)) continue;
    float a[3], n[3];
    rtgs_face_unit_normal(vertices, faces, f, a, n);
    if (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) continue;
    if (src_normals) {
      const float sx = src_normals[i * 3], sy = src_normals[i * 3 + 1], sz = src_normals[i * 3 + 2];
      const float dot = (sx * n[0] + sy * n[1]) + sz * n[2];
      if (!(fabsf(dot) >= min_cos)) continue;
    }
    const double px = (double)points[i * 3], py = (double)points[i * 3 + 1], pz = (double)points[i * 3 + 2];
    const double nx = (double)n[0], ny = (double)n[1], nz = (double)n[2];
    const double qx = px - (double)c.x, qy = py - (double)c.y, qz = pz - (double)c.z;
    const double ex = px - (double)a[0], ey = py - (double)a[1], ez = pz - (double)a[2];
    const double r = (nx * ex + ny * ey) + nz * ez;
    double J[6];
    J[0] = qy * nz - qz * ny;
    J[1] = qz * nx - qx * nz;
    J[2] = qx * ny - qy * nx;
    J[3] = nx; J[4] = ny; J[5] = nz;
    int k = 0;
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
      for (int v = u; v < 6; ++v) { acc[k] = acc[k] + J[u] * J[v]; ++k; }
#pragma unroll
    for (int u = 0; u < 6; ++u) acc[21 + u] = acc[21 + u] + J[u] * r;
    acc[27] = acc[27] + r * r;
    acc[28] = acc[28] + (double)dd;
    acc[29] = acc[29] + 1.0;
  }
  tree(acc, lds, partial + (int64_t)blockIdx.x * OUT);
}

__global__ void __launch_bounds__(NT) total_kernel(const double* __restrict__ partial, int64_t chunks, double* __restrict__ out) {
  __shared__ double lds[WAVES * OUT];
  double acc[OUT];
#pragma unroll
  for (int k = 0; k < OUT; ++k) acc[k] = 0.0;
  for (int64_t ch = threadIdx.x; ch < chunks; ch += NT) {
#pragma unroll
    for (int k = 0; k < OUT; ++k) acc[k] = acc[k] + partial[ch * OUT + k];
  }
  tree(acc, lds, out);
}

}  // namespace rtgs_mesh_register_k

extern "C" {

using namespace rtgs_mesh_register_k;

size_t rtgs_mesh_register_scratch_bytes(int64_t N) {
  if (N <= 0 || N >= 0x80000000LL) return 0;
  return (size_t)((N + CHUNK - 1) / CHUNK) * OUT * sizeof(double);
}

int rtgs_mesh_register_accumulate(const float* points, const int32_t* face, const float* d2, const float* src_normals, int64_t N,
                                  const float* vertices, int64_t V, const int32_t* faces, int64_t F, const float* center_host,
                                  float max_d2, float min_cos, void* scratch, double* out, void* stream) {
  if (N < 0 || N >= 0x80000000LL || V <= 0 || F <= 0 || !vertices || !faces || !center_host || !out) return -1;
  if (N > 0 && (!points || !face || !d2 || !scratch)) return -1;
  const int64_t chunks = (N + CHUNK - 1) / CHUNK;                                  // < 2^21
  const Center c = {center_host[0], center_host[1], center_host[2]};
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)scratch;
  if (chunks > 0)
    hipLaunchKernelGGL(chunks_kernel, dim3((unsigned)chunks), dim3(NT), 0, s, points, face, d2, src_normals, N, vertices, faces, F, c,
                       max_d2, min_cos, partial);
  hipLaunchKernelGGL(total_kernel, dim3(1), dim3(NT), 0, s, (const double*)partial, chunks, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
