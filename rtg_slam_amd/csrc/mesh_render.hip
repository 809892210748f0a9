// gfx950 kernels + C ABI of the mesh renderer (include/rtgs_slam.h, "mesh render"): the depth map and the face map of an indexed
// triangle mesh at a pinhole pose.  No counterpart in the reference; tests/mesh_render_reference.py restates it in numpy and is
// the definition, matched bit for bit.  Built with -ffp-contract=off (Makefile EXTRA_mesh_render): every float step below is one
// correctly rounded operation, in the definition's order.
//
// One call, four launches on the caller's stream, no host read:
// clear      one thread per pixel: its 64-bit key = all ones; thread 0 also zeroes the queue's counter.
// faces      one thread per face.  The face setup (setup_face): gather the three corners, project them (the chain of
//            visibility.hip's add_kernel), the near test, the box - clamped in FLOAT, converted to integers only once it is
//            known to lie inside the image -, the three edges ordered lexicographically with their signs.  A face whose box
//            holds at most small_max pixels is walked by its thread.  A larger one is appended to a queue in the scratch: one
//            integer atomic add per wave (ballot, prefix count), a slot is written only when it is below F.
// large      a fixed grid of waves strides over the queue up to the device-side count, one face per wave: the setup again (the
//            same code, so the same bits), then the 64 lanes walk the box's pixels in row-major order.
// resolve    one thread per pixel: key -> depth and face (0 and -1 where the key is still all ones).
//
// A pixel's update is a plain 8-byte load of its key and an atomicMin(unsigned long long) only when the new key is smaller.  Keys
// only fall during a render, so a stale load can only be LARGER than the truth: at worst an atomic that changes nothing.  The
// smallest key (bits(z) << 32 | face) wins whatever order the faces arrive in: the picture depends neither on the queue's order
// nor on small_max.
//
// The colour pass (rtgs_mesh_shade) is a fifth kernel in a call of its own, after the face map exists: shade_kernel, below the
// four above, with its definition in tests/mesh_shade_reference.py.
//
// Index range: the caller guarantees 0 <= faces[i] < V (rtg_slam_amd/evaluation.py checks it once, when the mesh is given).
// Element indices are 64-bit: 3 V and 3 F can pass 2^31.
#include "../../include/rtgs_slam.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace rtgs_mesh_render_k {

constexpr int NT = 256;
constexpr int WAVE = 64;
constexpr int LARGE_BLOCKS = 2048;                         // x 4 waves: the fixed grid of the large-face kernel
constexpr unsigned long long EMPTY = ~0ull;
constexpr size_t COUNTER_BYTES = 16;

struct View {
  float m[12];                 // world-to-camera, the top three rows
  float fx, fy, cx, cy;
  int H, W;
  float near;
};

struct Edge {                  // the edge s -> e with s before e in (u, v) order; flip: the face walks it the other way
  float su, sv, du, dv;
  bool flip;
};

struct Face {
  Edge e0, e1, e2;             // b -> c, c -> a, a -> b
  float iza, izb, izc;
  int x0, y0, bw, bh;          // the box: columns x0 .. x0 + bw - 1, rows y0 .. y0 + bh - 1, inside the image
};

inline bool grid_for(int64_t n, unsigned* blocks) {
  const int64_t b = (n + NT - 1) / NT;
  if (b > 0x7fffffffLL) return false;
  *blocks = (unsigned)b;
  return true;
}

__device__ __forceinline__ bool project(const float* __restrict__ vertices, int64_t i, const View& f, float* u, float* v, float* iz) {
  const float x = vertices[i * 3], y = vertices[i * 3 + 1], z = vertices[i * 3 + 2];
  const float xc = ((f.m[0] * x + f.m[1] * y) + f.m[2] * z) + f.m[3];
  const float yc = ((f.m[4] * x + f.m[5] * y) + f.m[6] * z) + f.m[7];
  const float zc = ((f.m[8] * x + f.m[9] * y) + f.m[10] * z) + f.m[11];
  if (!(zc > f.near)) return false;                                                        // behind the near plane, or NaN
  *u = f.fx * xc / zc + f.cx;
  *v = f.fy * yc / zc + f.cy;
  *iz = 1.0f / zc;
  return fabsf(*u) < INFINITY && fabsf(*v) < INFINITY;                                     // false for NaN too
}

// false: the two ends project to one point, the face is degenerate
__device__ __forceinline__ bool make_edge(float pu, float pv, float qu, float qv, Edge* e) {
  if (pu == qu && pv == qv) return false;
  e->flip = qu < pu || (qu == pu && qv < pv);
  const float su = e->flip ? qu : pu, sv = e->flip ? qv : pv;
  const float eu = e->flip ? pu : qu, ev = e->flip ? pv : qv;
  e->su = su; e->sv = sv;
  e->du = eu - su; e->dv = ev - sv;
  return true;
}

__device__ __forceinline__ float edge_at(const Edge& e, float px, float py) {
  const float v = e.du * (py - e.sv) - e.dv * (px - e.su);
  return e.flip ? -v : v;
}

__device__ __forceinline__ bool setup_face(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t i,
                                           const View& f, Face* out) {
  const int64_t a = faces[i * 3], b = faces[i * 3 + 1], c = faces[i * 3 + 2];
  float au, av, bu, bv, cu, cv;
  if (!project(vertices, a, f, &au, &av, &out->iza)) return false;
  if (!project(vertices, b, f, &bu, &bv, &out->izb)) return false;
  if (!project(vertices, c, f, &cu, &cv, &out->izc)) return false;
  // every u, v is finite here; the clamps happen in float, the conversions only once the box is known to lie in the image
  const float x0 = fmaxf(ceilf(fminf(fminf(au, bu), cu)), 0.0f), x1 = fminf(floorf(fmaxf(fmaxf(au, bu), cu)), (float)(f.W - 1));
  const float y0 = fmaxf(ceilf(fminf(fminf(av, bv), cv)), 0.0f), y1 = fminf(floorf(fmaxf(fmaxf(av, bv), cv)), (float)(f.H - 1));
  if (!(x0 <= x1 && y0 <= y1)) return false;
  if (!make_edge(bu, bv, cu, cv, &out->e0) || !make_edge(cu, cv, au, av, &out->e1) || !make_edge(au, av, bu, bv, &out->e2)) return false;
  out->x0 = (int)x0; out->y0 = (int)y0;
  out->bw = (int)x1 - out->x0 + 1; out->bh = (int)y1 - out->y0 + 1;
  return true;
}

__device__ __forceinline__ void shade(const Face& t, int px, int py, int W, uint32_t face, unsigned long long* __restrict__ keys) {
  const float fx = (float)px, fy = (float)py;
  const float w0 = edge_at(t.e0, fx, fy), w1 = edge_at(t.e1, fx, fy), w2 = edge_at(t.e2, fx, fy);
  const float area = (w0 + w1) + w2;
  const bool in = (w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f && area > 0.0f) || (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f && area < 0.0f);
  if (!in) return;
  const float z = 1.0f / (((w0 * t.iza + w1 * t.izb) + w2 * t.izc) / area);
  if (!(z > 0.0f && z < INFINITY)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | face;
  unsigned long long* p = keys + ((int64_t)py * W + px);
  if (key < *(volatile unsigned long long*)p) atomicMin(p, key);
}

__global__ void __launch_bounds__(NT) clear_kernel(unsigned long long* __restrict__ keys, int64_t n, uint32_t* __restrict__ counter) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i == 0) *counter = 0u;
  if (i < n) keys[i] = EMPTY;
}

__global__ void __launch_bounds__(NT) faces_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t F, View f,
                                                   int32_t small_max, unsigned long long* __restrict__ keys,
                                                   uint32_t* __restrict__ counter, uint32_t* __restrict__ queue) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  Face t;
  const bool ok = i < F && setup_face(vertices, faces, i, f, &t);
  const bool large = ok && (int64_t)t.bw * t.bh > (int64_t)small_max;
  // every lane of the wave reaches the ballot: nothing above returns
  const unsigned long long mask = __ballot(large);
  if (mask != 0ull) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0u;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = (uint32_t)__shfl((int)base, leader, WAVE);
    if (large) {
      const uint64_t slot = (uint64_t)base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (slot < (uint64_t)F) queue[slot] = (uint32_t)i;                                   // always true: a face enters once
    }
  }
  if (!ok || large) return;
  for (int y = 0; y < t.bh; ++y)
    for (int x = 0; x < t.bw; ++x) shade(t, t.x0 + x, t.y0 + y, f.W, (uint32_t)i, keys);
}

__global__ void __launch_bounds__(NT) large_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t F, View f,
                                                   unsigned long long* __restrict__ keys, const uint32_t* __restrict__ counter,
                                                   const uint32_t* __restrict__ queue) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wave = (blockIdx.x * NT + threadIdx.x) / WAVE;
  const uint32_t waves = gridDim.x * (NT / WAVE);
  uint32_t count = *counter;
  if ((int64_t)count > F) count = (uint32_t)F;
  for (uint32_t q = wave; q < count; q += waves) {
    const int64_t i = queue[q];
    if (i >= F) continue;
    Face t;
    if (!setup_face(vertices, faces, i, f, &t)) continue;                                  // cannot happen: it was queued
    const uint32_t n = (uint32_t)t.bw * (uint32_t)t.bh, bw = (uint32_t)t.bw;              // <= H W < 2^31
    for (uint32_t k = lane; k < n; k += WAVE) shade(t, t.x0 + (int)(k % bw), t.y0 + (int)(k / bw), f.W, (uint32_t)i, keys);
  }
}

__global__ void __launch_bounds__(NT) resolve_kernel(const unsigned long long* __restrict__ keys, int64_t n, float* __restrict__ depth,
                                                     int32_t* __restrict__ face) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  const bool hit = k != EMPTY;
  depth[i] = hit ? __uint_as_float((uint32_t)(k >> 32)) : 0.0f;
  face[i] = hit ? (int32_t)(uint32_t)(k & 0xffffffffull) : -1;
}

inline size_t keys_bytes(int32_t H, int32_t W) { return (size_t)H * (size_t)W * sizeof(unsigned long long); }

// ---- the colour pass (rtgs_mesh_shade; tests/mesh_shade_reference.py is its definition) ----
// One thread per pixel of a finished face map, a wave per 64 consecutive pixels of one row: the face's setup again (the same
// code as the rasteriser's, so the very edge values whose signs admitted the pixel), the perspective-correct barycentrics, then
// the three corner colours, or four texels of the atlas.  No LDS, no atomics; every read is guarded by 0 <= face < F, the
// caller's 0 <= faces[i] < V and the clamp of the texel coordinates, so any face map is safe.

struct Source {
  const float* colors;         // [V][3], or null: the texture is the source
  const float* uv;             // [F][3][2], y down
  const uint8_t* texture;      // [Ht][Wt][3]
  int Ht, Wt;
  float bg[3];
};

__device__ __forceinline__ float clamp_to(float x, float hi) { return fminf(fmaxf(x, 0.0f), hi); }      // NaN gives 0

__device__ __forceinline__ float texel(const uint8_t* __restrict__ texture, int64_t Wt, int y, int x, int c) {
  return (float)texture[((int64_t)y * Wt + x) * 3 + c] / 255.0f;
}

__global__ void __launch_bounds__(NT) shade_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t F, View f,
                                                   const int32_t* __restrict__ face_map, Source src, int32_t chunks,
                                                   float* __restrict__ out) {
  const int64_t wave = ((int64_t)blockIdx.x * NT + threadIdx.x) / WAVE;                    // (row, chunk of 64 columns)
  const int64_t row = wave / chunks;
  const int px = (int)(wave % chunks) * WAVE + (int)(threadIdx.x & (WAVE - 1));
  if (row >= f.H || px >= f.W) return;
  const int py = (int)row;
  const int64_t n = (int64_t)f.H * f.W, p = row * f.W + px;
  float c[3] = {src.bg[0], src.bg[1], src.bg[2]};
  const int64_t i = face_map[p];
  Face t;
  if (i >= 0 && i < F && setup_face(vertices, faces, i, f, &t)) {
    const float x = (float)px, y = (float)py;
    const float b0 = edge_at(t.e0, x, y) * t.iza, b1 = edge_at(t.e1, x, y) * t.izb, b2 = edge_at(t.e2, x, y) * t.izc;
    const float s = (b0 + b1) + b2;
    const float l0 = b0 / s, l1 = b1 / s, l2 = b2 / s;
    if (fabsf(l0) < INFINITY && fabsf(l1) < INFINITY && fabsf(l2) < INFINITY) {            // false for NaN too
      if (src.colors) {
        const int64_t va = faces[i * 3], vb = faces[i * 3 + 1], vc = faces[i * 3 + 2];
        for (int k = 0; k < 3; ++k)
          c[k] = clamp_to((l0 * src.colors[va * 3 + k] + l1 * src.colors[vb * 3 + k]) + l2 * src.colors[vc * 3 + k], 1.0f);
      } else {
        const float* q = src.uv + i * 6;
        const float tu = (l0 * q[0] + l1 * q[2]) + l2 * q[4], tv = (l0 * q[1] + l1 * q[3]) + l2 * q[5];
        const float X = clamp_to(tu * (float)src.Wt - 0.5f, (float)(src.Wt - 1));
        const float Y = clamp_to(tv * (float)src.Ht - 0.5f, (float)(src.Ht - 1));
        const float fx0 = floorf(X), fy0 = floorf(Y);
        const float tx = X - fx0, ty = Y - fy0;
        const int ix = (int)fx0, iy = (int)fy0;                                            // 0 .. Wt - 1, 0 .. Ht - 1
        const int ix1 = ix + 1 < src.Wt ? ix + 1 : src.Wt - 1, iy1 = iy + 1 < src.Ht ? iy + 1 : src.Ht - 1;
        for (int k = 0; k < 3; ++k) {
          const float c00 = texel(src.texture, src.Wt, iy, ix, k), c10 = texel(src.texture, src.Wt, iy, ix1, k);
          const float c01 = texel(src.texture, src.Wt, iy1, ix, k), c11 = texel(src.texture, src.Wt, iy1, ix1, k);
          const float top = c00 + tx * (c10 - c00), bot = c01 + tx * (c11 - c01);
          c[k] = top + ty * (bot - top);
        }
      }
    }
  }
  out[p] = c[0];
  out[n + p] = c[1];
  out[2 * n + p] = c[2];
}

}  // namespace rtgs_mesh_render_k

extern "C" {

using namespace rtgs_mesh_render_k;

size_t rtgs_mesh_render_scratch_bytes(int64_t V, int64_t F, int32_t H, int32_t W) {
  (void)V;                                                                                 // the corners are projected per face
  if (F < 0 || F >= 0x80000000LL || H <= 0 || W <= 0 || (int64_t)H * W >= 0x80000000LL) return 0;
  return keys_bytes(H, W) + COUNTER_BYTES + (size_t)F * sizeof(uint32_t);
}

int rtgs_mesh_render(const float* vertices, int64_t V, const int32_t* faces, int64_t F, int32_t H, int32_t W, float fx, float fy,
                     float cx, float cy, const float* w2c12_host, float near, int32_t small_max, void* scratch, float* depth,
                     int32_t* face, void* stream) {
  if (V < 0 || F < 0 || F >= 0x80000000LL || H <= 0 || W <= 0 || (int64_t)H * W >= 0x80000000LL) return -1;
  if (!w2c12_host || !(near > 0.0f) || small_max < 0 || !scratch || !depth || !face) return -1;
  if (F > 0 && (!faces || !vertices || V == 0)) return -1;
  View f;
  for (int k = 0; k < 12; ++k) f.m[k] = w2c12_host[k];
  f.fx = fx; f.fy = fy; f.cx = cx; f.cy = cy;
  f.H = H; f.W = W;
  f.near = near;
  const int64_t n = (int64_t)H * W;
  unsigned long long* keys = (unsigned long long*)scratch;
  uint32_t* counter = (uint32_t*)((char*)scratch + keys_bytes(H, W));
  uint32_t* queue = (uint32_t*)((char*)scratch + keys_bytes(H, W) + COUNTER_BYTES);
  unsigned pixel_blocks, face_blocks = 0;
  if (!grid_for(n, &pixel_blocks) || (F > 0 && !grid_for(F, &face_blocks))) return -1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(clear_kernel, dim3(pixel_blocks), dim3(NT), 0, s, keys, n, counter);
  if (F > 0) {
    hipLaunchKernelGGL(faces_kernel, dim3(face_blocks), dim3(NT), 0, s, vertices, faces, F, f, small_max, keys, counter, queue);
    const int64_t one_wave_each = (F + NT / WAVE - 1) / (NT / WAVE);
    const unsigned large_blocks = (unsigned)(one_wave_each < LARGE_BLOCKS ? one_wave_each : LARGE_BLOCKS);
    hipLaunchKernelGGL(large_kernel, dim3(large_blocks), dim3(NT), 0, s, vertices, faces, F, f, keys, counter, queue);
  }
  hipLaunchKernelGGL(resolve_kernel, dim3(pixel_blocks), dim3(NT), 0, s, keys, n, depth, face);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_mesh_shade(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int32_t* face_map, int32_t H, int32_t W,
                    float fx, float fy, float cx, float cy, const float* w2c12_host, float near, const float* colors, const float* uv,
                    const uint8_t* texture, int32_t Ht, int32_t Wt, const float* background3_host, float* out, void* stream) {
  if (V < 0 || F < 0 || F >= 0x80000000LL || H <= 0 || W <= 0 || (int64_t)H * W >= 0x80000000LL) return -1;
  if (!w2c12_host || !(near > 0.0f) || !face_map || !background3_host || !out) return -1;
  if (F > 0 && (!faces || !vertices || V == 0)) return -1;
  if ((uv != nullptr) != (texture != nullptr)) return -1;
  if ((colors != nullptr) == (uv != nullptr)) return -1;                                   // one source, not none and not both
  if (uv && (Ht < 1 || Wt < 1 || Ht > RTGS_MESH_TEXTURE_MAX_SIDE || Wt > RTGS_MESH_TEXTURE_MAX_SIDE)) return -1;
  View f;
  for (int k = 0; k < 12; ++k) f.m[k] = w2c12_host[k];
  f.fx = fx; f.fy = fy; f.cx = cx; f.cy = cy;
  f.H = H; f.W = W;
  f.near = near;
  Source src;
  src.colors = colors; src.uv = uv; src.texture = texture;
  src.Ht = uv ? Ht : 1; src.Wt = uv ? Wt : 1;
  for (int k = 0; k < 3; ++k) src.bg[k] = background3_host[k];
  const int32_t chunks = (W + WAVE - 1) / WAVE;                                            // waves per row
  unsigned blocks;
  if (!grid_for((int64_t)H * chunks * WAVE, &blocks)) return -1;                           // H chunks <= H W < 2^31 waves
  hipLaunchKernelGGL(shade_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, vertices, faces, F, f, face_map, src, chunks, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
