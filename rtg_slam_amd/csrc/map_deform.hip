// rtgs_map_deform (include/rtgs_slam.h): the map moves with its frames.  After a loop closure every frame f has a rigid correction
// D(f) = T'_f T_f^-1; a Gaussian is moved by the correction of the frame that added it (its add_tick).  One lane per row, no
// atomics, no host read; tests/map_deform_reference.py restates the float32 chain below and the kernel matches it bit for bit
// (fmaf is written out: the contraction the compiler may or may not do is not part of the definition).
//
// Traffic per row: 12 B xyz + 16 B rotation in, the same out, 4 or 8 B of tick, and one 64-B table row - rows added by one frame
// sit next to each other, so the lanes of a wave mostly gather the same table row.  xyz is read as three scalar loads (the rows
// are 12 B apart, a wave's 768 B are contiguous); the rotation and the table row are float4.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtgs_slam.h"

namespace rtgs {

template <typename TickT>
__global__ void __launch_bounds__(256) map_deform_kernel(float* __restrict__ xyz, float4* __restrict__ raw8, const TickT* __restrict__ tick,
                                                         long long N, const float4* __restrict__ table, int n_frames) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  long long f = (long long)tick[i];
  f = f < 0 ? 0 : (f > (long long)n_frames - 1 ? (long long)n_frames - 1 : f);
  const float4 r0 = table[4 * f], r1 = table[4 * f + 1], r2 = table[4 * f + 2], q = table[4 * f + 3];
  // a row whose correction is exactly the identity is not written: it stays bit-identical, -0.0 included
  const bool identity = r0.x == 1.0f && r0.y == 0.0f && r0.z == 0.0f && r0.w == 0.0f && r1.x == 0.0f && r1.y == 1.0f && r1.z == 0.0f &&
                        r1.w == 0.0f && r2.x == 0.0f && r2.y == 0.0f && r2.z == 1.0f && r2.w == 0.0f && q.x == 1.0f && q.y == 0.0f &&
                        q.z == 0.0f && q.w == 0.0f;
  if (identity) return;
  const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  xyz[3 * i] = fmaf(r0.x, x, fmaf(r0.y, y, fmaf(r0.z, z, r0.w)));
  xyz[3 * i + 1] = fmaf(r1.x, x, fmaf(r1.y, y, fmaf(r1.z, z, r1.w)));
  xyz[3 * i + 2] = fmaf(r2.x, x, fmaf(r2.y, y, fmaf(r2.z, z, r2.w)));
  // q' = q_D (x) q_raw, Hamilton product of (w, x, y, z); q_D is a unit quaternion, so the norm of the raw one is kept
  const float4 b = raw8[2 * i + 1];
  const float aw = q.x, ax = q.y, ay = q.z, az = q.w, bw = b.x, bx = b.y, by = b.z, bz = b.w;
  float4 o;
  o.x = fmaf(-az, bz, fmaf(-ay, by, fmaf(-ax, bx, aw * bw)));
  o.y = fmaf(-az, by, fmaf(ay, bz, fmaf(ax, bw, aw * bx)));
  o.z = fmaf(az, bx, fmaf(ay, bw, fmaf(-ax, bz, aw * by)));
  o.w = fmaf(az, bw, fmaf(-ay, bx, fmaf(ax, by, aw * bz)));
  raw8[2 * i + 1] = o;
}

}  // namespace rtgs

extern "C" int rtgs_map_deform(float* xyz, float* raw8, const void* tick, int32_t tick_kind, int64_t N, const float* table,
                               int32_t n_frames, void* stream) {
  if (N < 0 || N > RTGS_MAP_DEFORM_MAX_ROWS || n_frames < 1 || (tick_kind != 0 && tick_kind != 1)) return -1;
  if (N == 0) return 0;
  if (!xyz || !raw8 || !tick || !table) return -1;
  if (((uintptr_t)raw8 & 15) || ((uintptr_t)table & 15)) return -1;
  const dim3 grid((unsigned)((N + 255) / 256)), block(256);
  if (tick_kind == 0)
    hipLaunchKernelGGL(rtgs::map_deform_kernel<int32_t>, grid, block, 0, (hipStream_t)stream, xyz, (float4*)raw8, (const int32_t*)tick,
                       (long long)N, (const float4*)table, (int)n_frames);
  else
    hipLaunchKernelGGL(rtgs::map_deform_kernel<int64_t>, grid, block, 0, (hipStream_t)stream, xyz, (float4*)raw8, (const int64_t*)tick,
                       (long long)N, (const float4*)table, (int)n_frames);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
