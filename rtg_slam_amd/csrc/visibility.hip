// gfx950 kernels + C ABI of the visibility cull (include/rtgs_slam.h, "visibility"): which vertices of a mesh a sequence of
// depth frames saw, and which faces that leaves.  No counterpart in the reference; tests/visibility_reference.py restates both
// in numpy and is the definition, matched bit for bit.  Built with -ffp-contract=off (Makefile EXTRA_visibility): every float
// step below is one correctly rounded operation, in the order of tsdf.hip's project_voxel (the same chain, on a point that is
// given and not a voxel centre).
//
// add        one thread per point.  The view (the 12 world-to-camera entries, the intrinsics, the image size, the tolerance)
//            is a kernel argument: uniform, so it lives in scalar registers.  A thread loads its point (12 B; a wave's 768 B
//            are contiguous), projects it, and only a point in front of the camera and inside the image goes to memory again:
//            one gather from the depth image (a 1200 x 680 float image is 3.3 MB: it stays in L2), and, when the point is
//            neither in a hole nor more than `tolerance` behind the measured surface, a read and a write of its own counter.
//            views[i] has one owner, thread i: no atomics.  No LDS, no barrier, a handful of registers.
// keep_faces one thread per face: three gathers from views, one store.
//
// Index range: the caller guarantees 0 <= faces[i] < V (rtg_slam_amd/evaluation.py checks it once, when the mesh is given).
// Element indices are 64-bit: 3 N and 3 F can pass 2^31.
#include "../../include/rtgs_slam.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtgs_visibility {

constexpr int NT = 256;

struct View {
  float m[12];                 // world-to-camera, the top three rows
  float fx, fy, cx, cy;
  int H, W;
  float tolerance;
};

inline bool grid_for(int64_t n, unsigned* blocks) {
  const int64_t b = (n + NT - 1) / NT;
  if (b > 0x7fffffffLL) return false;
  *blocks = (unsigned)b;
  return true;
}

__global__ void __launch_bounds__(NT) add_kernel(const float* __restrict__ points, int64_t N, const float* __restrict__ depth,
                                                 View f, int32_t* __restrict__ views) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= N) return;
  const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
  const float xc = ((f.m[0] * x + f.m[1] * y) + f.m[2] * z) + f.m[3];
  const float yc = ((f.m[4] * x + f.m[5] * y) + f.m[6] * z) + f.m[7];
  const float zc = ((f.m[8] * x + f.m[9] * y) + f.m[10] * z) + f.m[11];
  if (!(zc > 0.0f)) return;                                                               // behind the camera, or NaN
  const float u = f.fx * xc / zc + f.cx;
  const float v = f.fy * yc / zc + f.cy;
  const float pu = floorf(u + 0.5f), pv = floorf(v + 0.5f);
  if (!(pu >= 0.0f && pu < (float)f.W && pv >= 0.0f && pv < (float)f.H)) return;          // also drops NaN / inf
  const float d = depth[(int64_t)pv * f.W + (int64_t)pu];
  if (!(d > 0.0f)) return;                                                                // a hole sees nothing
  if (zc - d > f.tolerance) return;                                                       // behind what the sensor measured
  views[i] = views[i] + 1;
}

__global__ void __launch_bounds__(NT) keep_faces_kernel(const int32_t* __restrict__ faces, int64_t F, const int32_t* __restrict__ views,
                                                        int32_t min_views, int any_vertex, int32_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= F) return;
  const bool a = views[faces[i * 3]] >= min_views;
  const bool b = views[faces[i * 3 + 1]] >= min_views;
  const bool c = views[faces[i * 3 + 2]] >= min_views;
  keep[i] = (any_vertex ? (a || b || c) : (a && b && c)) ? 1 : 0;
}

}  // namespace rtgs_visibility

extern "C" {

using namespace rtgs_visibility;

int rtgs_visibility_add(const float* points, int64_t N, const float* depth, int32_t H, int32_t W, float fx, float fy, float cx,
                        float cy, const float* w2c12_host, float tolerance, int32_t* views, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || !w2c12_host || !(tolerance >= 0.0f)) return -1;
  if (N == 0) return 0;
  if (!points || !depth || !views) return -1;
  View f;
  for (int k = 0; k < 12; ++k) f.m[k] = w2c12_host[k];
  f.fx = fx; f.fy = fy; f.cx = cx; f.cy = cy;
  f.H = H; f.W = W;
  f.tolerance = tolerance;
  unsigned blocks;
  if (!grid_for(N, &blocks)) return -1;
  hipLaunchKernelGGL(add_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, points, N, depth, f, views);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_visibility_keep_faces(const int32_t* faces, int64_t F, const int32_t* views, int32_t min_views, int32_t any_vertex,
                               int32_t* keep, void* stream) {
  if (F < 0) return -1;
  if (F == 0) return 0;
  if (!faces || !views || !keep) return -1;
  unsigned blocks;
  if (!grid_for(F, &blocks)) return -1;
  hipLaunchKernelGGL(keep_faces_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, faces, F, views, min_views, (int)any_vertex,
                     keep);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
