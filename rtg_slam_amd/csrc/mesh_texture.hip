// gfx950 kernels + C ABI of the mesh texture bake (include/rtgs_slam.h, "mesh texture"): a per-face atlas of an indexed triangle
// mesh, baked from colour views.  No counterpart in the reference; tests/mesh_texture_reference.py restates every step in numpy
// and is the definition, matched bit for bit.  Built with -ffp-contract=off (Makefile EXTRA_mesh_texture): every float step below
// is one correctly rounded float32 operation in the order written; the projection chain is visibility.hip's.
//
// levels      one thread per face: the longest squared edge against ((2^l - 1) texel)^2, l = 1..max_level.
// face_layout one thread per face: the block origin (the Morton decode of the face's offset), the three texture coordinates, and
//             the face's bake record: 48 B = three float4 - the corner A, the edges B - A and C - A, the origin and the level.
// texel_face  one thread per atlas texel: its Morton code, a binary search of the sorted offsets.  Written once per atlas.
// bake_view   one thread per atlas texel, a wave's 64 texels consecutive in x.  The view (the 12 world-to-camera entries, the
//             camera centre, the intrinsics, the image size, the tolerance) is a kernel argument: uniform, so it lives in scalar
//             registers.  A thread reads its face index (4 B, coalesced); an unassigned texel ends there.  The face's record is
//             three 16 B gathers, one dependent step after the face index (not face -> indices -> corners), which a block's
//             texels share (one face has up to 4096 texels), so they hit L1 / L2.  Only a texel that passes every test touches
//             its accumulator: one 16 B read and one 16 B write.
//             acc[texel] has one owner, this thread: no atomics, and views accumulate in launch order.
// finish      one thread per texel: the colour (acc.rgb / w, or the vertex-colour blend, or nothing), three bytes and a flag.
//
// Index range: the caller guarantees 0 <= faces[i] < V, 0 <= order[i] < F, 1 <= levels[i] <= 6, and that texel_face and origin
// and record are what texel_face and face_layout wrote for this atlas.  Element indices are 64-bit.
#include "../../include/rtgs_slam.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace rtgs_mesh_texture {

constexpr int NT = 256;
constexpr int MAX_SIDE = RTGS_MESH_TEXTURE_MAX_SIDE;
constexpr int MAX_LEVEL = RTGS_MESH_TEXTURE_MAX_LEVEL;

struct View {
  float m[12];                 // world-to-camera, the top three rows
  float o[3];                  // the camera centre in the mesh's frame
  float fx, fy, cx, cy;
  int H, W;
  float tolerance, min_cos2;
};

inline bool grid_for(int64_t n, unsigned* blocks) {
  const int64_t b = (n + NT - 1) / NT;
  if (b > 0x7fffffffLL) return false;
  *blocks = (unsigned)b;
  return true;
}

// x -> the even bits of the result (x < 2^16)
__device__ __forceinline__ uint32_t part1by1(uint32_t v) {
  v &= 0x0000ffffu;
  v = (v | (v << 8)) & 0x00ff00ffu;
  v = (v | (v << 4)) & 0x0f0f0f0fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}

__device__ __forceinline__ uint32_t compact1by1(uint32_t v) {
  v &= 0x55555555u;
  v = (v | (v >> 1)) & 0x33333333u;
  v = (v | (v >> 2)) & 0x0f0f0f0fu;
  v = (v | (v >> 4)) & 0x00ff00ffu;
  v = (v | (v >> 8)) & 0x0000ffffu;
  return v;
}

__device__ __forceinline__ float dist2(const float* p, const float* q) {
  const float dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ float dot3(const float* p, const float* q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }

__device__ __forceinline__ void load_corners(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t f, float* a,
                                             float* b, float* c) {
  const int64_t ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
  for (int k = 0; k < 3; ++k) {
    a[k] = vertices[ia * 3 + k];
    b[k] = vertices[ib * 3 + k];
    c[k] = vertices[ic * 3 + k];
  }
}

// (i, j) inside the face's block, mirrored across the hypotenuse into the triangle -> a = i / (s - 1), b = j / (s - 1)
__device__ __forceinline__ void texel_ab(int x, int y, int x0, int y0, int level, float* a, float* b) {
  const int s1 = (1 << level) - 1;
  int i = x - x0, j = y - y0;
  if (i + j > s1) {
    const int t = s1 - j;
    j = s1 - i;
    i = t;
  }
  *a = (float)i / (float)s1;
  *b = (float)j / (float)s1;
}

__global__ void __launch_bounds__(NT) levels_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t F,
                                                    float texel, int max_level, int32_t* __restrict__ levels,
                                                    int32_t* __restrict__ capped) {
  const int64_t f = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (f >= F) return;
  float a[3], b[3], c[3];
  load_corners(vertices, faces, f, a, b, c);
  bool finite = true;
  for (int k = 0; k < 3; ++k) finite = finite && isfinite(a[k]) && isfinite(b[k]) && isfinite(c[k]);
  int level = 1, cap = 0;
  if (finite) {
    const float L = fmaxf(fmaxf(dist2(a, b), dist2(b, c)), dist2(c, a));
    level = 0;
    for (int l = 1; l <= max_level; ++l) {
      const float t = (float)((1 << l) - 1) * texel;
      if (t * t >= L) { level = l; break; }
    }
    if (level == 0) { level = max_level; cap = 1; }
  }
  levels[f] = level;
  capped[f] = cap;
}

__global__ void __launch_bounds__(NT) face_layout_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                         const int64_t* __restrict__ offset, const int32_t* __restrict__ levels,
                                                         int64_t F, float Wt, float Ht, int32_t* __restrict__ origin,
                                                         float* __restrict__ uv, float4* __restrict__ record) {
  const int64_t f = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (f >= F) return;
  const uint32_t code = (uint32_t)offset[f];
  const uint32_t x0 = compact1by1(code), y0 = compact1by1(code >> 1);
  origin[f * 2] = (int32_t)x0;
  origin[f * 2 + 1] = (int32_t)y0;
  const float s = (float)(1 << levels[f]);
  const float xf = (float)x0, yf = (float)y0;
  const float u0 = (xf + 0.5f) / Wt, v0 = (yf + 0.5f) / Ht;
  const float u1 = ((xf + s) - 0.5f) / Wt, v1 = ((yf + s) - 0.5f) / Ht;
  float* o = uv + f * 6;
  o[0] = u0; o[1] = v0;
  o[2] = u1; o[3] = v0;
  o[4] = u0; o[5] = v1;
  float a[3], b[3], c[3];
  load_corners(vertices, faces, f, a, b, c);
  const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
  const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
  record[f * 3] = make_float4(a[0], a[1], a[2], e1x);
  record[f * 3 + 1] = make_float4(e1y, e1z, e2x, e2y);
  record[f * 3 + 2] = make_float4(e2z, __int_as_float((int)x0), __int_as_float((int)y0), __int_as_float(levels[f]));
}

__global__ void __launch_bounds__(NT) texel_face_kernel(const int64_t* __restrict__ sorted_offset, const int32_t* __restrict__ order,
                                                        int64_t F, int64_t T, int Wt, int64_t n, int32_t* __restrict__ texel_face) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = (uint32_t)(i % Wt), y = (uint32_t)(i / Wt);
  const int64_t code = (int64_t)(part1by1(x) | (part1by1(y) << 1));
  int32_t face = -1;
  if (code < T) {
    int64_t lo = 0, hi = F;                        // the last slot with sorted_offset <= code; sorted_offset[0] = 0
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (sorted_offset[mid] <= code) lo = mid; else hi = mid;
    }
    face = order[lo];
  }
  texel_face[i] = face;
}

__global__ void __launch_bounds__(NT) bake_view_kernel(const int32_t* __restrict__ texel_face, int Wt, int64_t n,
                                                       const float4* __restrict__ record, const float* __restrict__ color,
                                                       const float* __restrict__ depth, View f, float4* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int64_t face = texel_face[i];
  if (face < 0) return;
  const float4 r0 = record[face * 3], r1 = record[face * 3 + 1], r2 = record[face * 3 + 2];
  float ta, tb;
  texel_ab((int)(i % Wt), (int)(i / Wt), __float_as_int(r2.y), __float_as_int(r2.z), __float_as_int(r2.w), &ta, &tb);
  const float A[3] = {r0.x, r0.y, r0.z}, e1[3] = {r0.w, r1.x, r1.y}, e2[3] = {r1.z, r1.w, r2.x};
  float p[3];
  for (int k = 0; k < 3; ++k) p[k] = (A[k] + ta * e1[k]) + tb * e2[k];
  const float xc = ((f.m[0] * p[0] + f.m[1] * p[1]) + f.m[2] * p[2]) + f.m[3];
  const float yc = ((f.m[4] * p[0] + f.m[5] * p[1]) + f.m[6] * p[2]) + f.m[7];
  const float zc = ((f.m[8] * p[0] + f.m[9] * p[1]) + f.m[10] * p[2]) + f.m[11];
  if (!(zc > 0.0f)) return;                                                               // behind the camera, or NaN
  const float u = f.fx * xc / zc + f.cx;
  const float v = f.fy * yc / zc + f.cy;
  const float x0 = floorf(u), y0 = floorf(v);
  if (!(x0 >= 0.0f && x0 <= (float)(f.W - 2) && y0 >= 0.0f && y0 <= (float)(f.H - 2))) return;   // the bilinear footprint; drops NaN / inf
  const float pu = floorf(u + 0.5f), pv = floorf(v + 0.5f);                               // inside the footprint
  const float d = depth[(int64_t)pv * f.W + (int64_t)pu];
  if (!(d > 0.0f)) return;                                                                // a hole: this view is not used here
  if (zc - d > f.tolerance) return;                                                       // behind the rendered surface
  float nrm[3], r[3];
  nrm[0] = e1[1] * e2[2] - e1[2] * e2[1];
  nrm[1] = e1[2] * e2[0] - e1[0] * e2[2];
  nrm[2] = e1[0] * e2[1] - e1[1] * e2[0];
  for (int k = 0; k < 3; ++k) r[k] = f.o[k] - p[k];
  const float nr = dot3(nrm, r);
  const float cos2 = (nr * nr) / (dot3(nrm, nrm) * dot3(r, r));
  if (!(cos2 >= f.min_cos2)) return;                                                      // grazing, or a face without area (NaN)
  const float w = cos2 / (zc * zc);
  const float tx = u - x0, ty = v - y0;
  const int64_t plane = (int64_t)f.H * f.W;
  const float* c00 = color + (int64_t)y0 * f.W + (int64_t)x0;
  float val[3];
  for (int k = 0; k < 3; ++k) {
    const float* q = c00 + k * plane;
    const float top = q[0] + tx * (q[1] - q[0]);
    const float bot = q[f.W] + tx * (q[f.W + 1] - q[f.W]);
    val[k] = top + ty * (bot - top);
  }
  float4 a4 = acc[i];
  a4.x = a4.x + w * val[0];
  a4.y = a4.y + w * val[1];
  a4.z = a4.z + w * val[2];
  a4.w = a4.w + w;
  acc[i] = a4;
}

__device__ __forceinline__ uint8_t to_byte(float c) {
  const float q = floorf(c * 255.0f + 0.5f);
  return (uint8_t)fminf(fmaxf(q, 0.0f), 255.0f);                                          // fmaxf(NaN, 0) = 0
}

__global__ void __launch_bounds__(NT) finish_kernel(const int32_t* __restrict__ texel_face, int Wt, int64_t n,
                                                    const int32_t* __restrict__ faces, const int32_t* __restrict__ levels,
                                                    const int32_t* __restrict__ origin, const float* __restrict__ colors,
                                                    const float4* __restrict__ acc, uint8_t* __restrict__ image,
                                                    uint8_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int64_t face = texel_face[i];
  float c[3] = {0.0f, 0.0f, 0.0f};
  uint8_t flag = 0;
  if (face >= 0) {
    const float4 a4 = acc[i];
    if (a4.w > 0.0f) {
      flag = 2;
      c[0] = a4.x / a4.w; c[1] = a4.y / a4.w; c[2] = a4.z / a4.w;
    } else if (colors) {
      flag = 1;
      float ta, tb;
      texel_ab((int)(i % Wt), (int)(i / Wt), origin[face * 2], origin[face * 2 + 1], levels[face], &ta, &tb);
      float A[3], B[3], C[3];
      load_corners(colors, faces, face, A, B, C);
      for (int k = 0; k < 3; ++k) c[k] = (A[k] + ta * (B[k] - A[k])) + tb * (C[k] - A[k]);
    } else {
      flag = 1;
      c[0] = c[1] = c[2] = 0.5f;
    }
  }
  image[i * 3] = to_byte(c[0]);
  image[i * 3 + 1] = to_byte(c[1]);
  image[i * 3 + 2] = to_byte(c[2]);
  flags[i] = flag;
}

inline bool atlas_ok(int32_t Wt, int32_t Ht) { return Wt >= 1 && Ht >= 1 && Wt <= MAX_SIDE && Ht <= MAX_SIDE; }

}  // namespace rtgs_mesh_texture

extern "C" {

using namespace rtgs_mesh_texture;

int rtgs_mesh_texture_levels(const float* vertices, const int32_t* faces, int64_t F, float texel, int32_t max_level, int32_t* levels,
                             int32_t* capped, void* stream) {
  if (F < 0 || !(texel > 0.0f) || !(texel < INFINITY) || max_level < 1 || max_level > MAX_LEVEL) return -1;
  if (F == 0) return 0;
  if (!vertices || !faces || !levels || !capped) return -1;
  unsigned blocks;
  if (!grid_for(F, &blocks)) return -1;
  hipLaunchKernelGGL(levels_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, vertices, faces, F, texel, (int)max_level, levels,
                     capped);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_mesh_texture_face_layout(const float* vertices, const int32_t* faces, const int64_t* offset, const int32_t* levels, int64_t F,
                                  int32_t Wt, int32_t Ht, int32_t* origin, float* uv, float* record, void* stream) {
  if (F < 0 || !atlas_ok(Wt, Ht)) return -1;
  if (F == 0) return 0;
  if (!vertices || !faces || !offset || !levels || !origin || !uv || !record) return -1;
  unsigned blocks;
  if (!grid_for(F, &blocks)) return -1;
  hipLaunchKernelGGL(face_layout_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, vertices, faces, offset, levels, F, (float)Wt,
                     (float)Ht, origin, uv, (float4*)record);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_mesh_texture_texel_face(const int64_t* sorted_offset, const int32_t* order, int64_t F, int64_t T, int32_t Wt, int32_t Ht,
                                 int32_t* texel_face, void* stream) {
  if (F < 1 || T < 0 || !atlas_ok(Wt, Ht) || !sorted_offset || !order || !texel_face) return -1;
  const int64_t n = (int64_t)Wt * Ht;
  unsigned blocks;
  if (!grid_for(n, &blocks)) return -1;
  hipLaunchKernelGGL(texel_face_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, sorted_offset, order, F, T, (int)Wt, n,
                     texel_face);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_mesh_texture_bake_view(const int32_t* texel_face, int32_t Wt, int32_t Ht, const float* record, const float* color,
                                const float* depth, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                                const float* w2c12_host, const float* centre_host, float tolerance, float min_cos2, float* acc,
                                void* stream) {
  if (!atlas_ok(Wt, Ht) || H <= 0 || W <= 0 || H > (1 << 24) || W > (1 << 24) || (int64_t)H * W >= 0x7fffffffLL || !w2c12_host ||
      !centre_host || !(tolerance >= 0.0f) || !(min_cos2 >= 0.0f))
    return -1;
  if (!texel_face || !record || !color || !depth || !acc) return -1;
  View f;
  for (int k = 0; k < 12; ++k) f.m[k] = w2c12_host[k];
  for (int k = 0; k < 3; ++k) f.o[k] = centre_host[k];
  f.fx = fx; f.fy = fy; f.cx = cx; f.cy = cy;
  f.H = H; f.W = W;
  f.tolerance = tolerance;
  f.min_cos2 = min_cos2;
  const int64_t n = (int64_t)Wt * Ht;
  unsigned blocks;
  if (!grid_for(n, &blocks)) return -1;
  hipLaunchKernelGGL(bake_view_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, texel_face, (int)Wt, n, (const float4*)record,
                     color, depth, f, (float4*)acc);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_mesh_texture_finish(const int32_t* texel_face, int32_t Wt, int32_t Ht, const int32_t* faces, const int32_t* levels,
                             const int32_t* origin, const float* colors, const float* acc, uint8_t* image, uint8_t* flags,
                             void* stream) {
  if (!atlas_ok(Wt, Ht) || !texel_face || !faces || !levels || !origin || !acc || !image || !flags) return -1;
  const int64_t n = (int64_t)Wt * Ht;
  unsigned blocks;
  if (!grid_for(n, &blocks)) return -1;
  hipLaunchKernelGGL(finish_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, texel_face, (int)Wt, n, faces, levels, origin, colors,
                     (const float4*)acc, image, flags);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
