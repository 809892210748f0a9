// The float32 unit normal of one face of an indexed mesh, shared by rtgs_mesh_distance_normals (csrc/mesh_distance.hip) and
// rtgs_mesh_register_accumulate (csrc/mesh_register.hip) so that both have the same bits.  Both files are built with
// -ffp-contract=off: every step is one correctly rounded float32 operation, in tests/mesh_distance_reference.py's
// face_unit_normals order.
#ifndef RTGS_MESH_FACE_NORMAL_H
#define RTGS_MESH_FACE_NORMAL_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// n = (b - a) x (c - a) / l, l = sqrt((x x + y y) + z z), when l > 0 and finite; (0, 0, 0) otherwise.  a: the face's first corner.
// The caller guarantees 0 <= f < F and 0 <= faces[.] < V.
__device__ __forceinline__ void rtgs_face_unit_normal(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t f,
                                                      float* __restrict__ a, float* __restrict__ n) {
  const int64_t ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
  const float ax = vertices[ia * 3], ay = vertices[ia * 3 + 1], az = vertices[ia * 3 + 2];
  const float e1x = vertices[ib * 3] - ax, e1y = vertices[ib * 3 + 1] - ay, e1z = vertices[ib * 3 + 2] - az;
  const float e2x = vertices[ic * 3] - ax, e2y = vertices[ic * 3 + 1] - ay, e2z = vertices[ic * 3 + 2] - az;
  const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
  const float l = sqrtf((cx * cx + cy * cy) + cz * cz);
  a[0] = ax; a[1] = ay; a[2] = az;
  n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
  if (l > 0.0f && l < INFINITY) { n[0] = cx / l; n[1] = cy / l; n[2] = cz / l; }
}

#endif  // RTGS_MESH_FACE_NORMAL_H
