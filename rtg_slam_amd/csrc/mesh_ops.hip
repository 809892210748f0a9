// gfx950 kernels + C ABI of the mesh clean-up (include/rtgs_slam.h, "mesh operations"): per-vertex normals, connected
// components with small-component removal, compaction, and vertex-clustering simplification of an indexed triangle mesh
// (vertices [V][3] float32, faces [F][3] int32, colours [V][3] float32) that already lies on the device after extract_mesh.
// No counterpart in the reference; tests/mesh_ops_reference.py restates every result in numpy and the kernels match it bit
// for bit.  Built with -ffp-contract=off (Makefile EXTRA_mesh_ops): every float step below is one correctly rounded operation.
//
// Nothing here adds floats atomically.  A sum that several faces or vertices contribute to is formed by ONE thread that
// walks the contributors in a fixed order (the caller's stable sort), so two runs are bit-equal.  The walks are dependent
// gathers and the union-find is integer atomics on global memory: latency-bound, sized by V and F, not by bytes.
//
// Index range: the caller guarantees 0 <= faces[i] < V (rtg_slam_amd/mesh_ops.py checks it before every call); the kernels
// trust it.  Element indices are 64-bit where 3 F can pass 2^31.
#include "../../include/rtgs_slam.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtgs_mesh {

constexpr int NT = 256;

inline bool grid_for(int64_t n, unsigned* blocks) {
  const int64_t b = (n + NT - 1) / NT;
  if (b > 0x7fffffffLL) return false;
  *blocks = (unsigned)b;
  return true;
}

// ---- a. vertex normals ----------------------------------------------------------------------------------------------

// area-weighted normal of one face: e1 x e2, each component two rounded products and a rounded difference
__device__ __forceinline__ void face_normal(const float* __restrict__ v, const int32_t* __restrict__ f, int64_t face, float n[3]) {
  const int64_t a = f[face * 3], b = f[face * 3 + 1], c = f[face * 3 + 2];
  const float p0x = v[a * 3], p0y = v[a * 3 + 1], p0z = v[a * 3 + 2];
  const float e1x = v[b * 3] - p0x, e1y = v[b * 3 + 1] - p0y, e1z = v[b * 3 + 2] - p0z;
  const float e2x = v[c * 3] - p0x, e2y = v[c * 3 + 1] - p0y, e2z = v[c * 3 + 2] - p0z;
  n[0] = e1y * e2z - e1z * e2y;
  n[1] = e1z * e2x - e1x * e2z;
  n[2] = e1x * e2y - e1y * e2x;
}

// one thread per vertex: its corners order[start[v] .. start[v + 1]) come in ascending corner index o = 3 f + k
__global__ void __launch_bounds__(NT) normals_kernel(const float* __restrict__ v, const int32_t* __restrict__ f,
                                                     const int64_t* __restrict__ order, const int64_t* __restrict__ start,
                                                     int64_t V, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= V) return;
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  const int64_t end = start[i + 1];
  for (int64_t j = start[i]; j < end; ++j) {
    float n[3];
    face_normal(v, f, order[j] / 3, n);
    sx = sx + n[0];
    sy = sy + n[1];
    sz = sz + n[2];
  }
  const float l = sqrtf((sx * sx + sy * sy) + sz * sz);
  const bool ok = l > 0.0f;
  out[i * 3] = ok ? sx / l : 0.0f;
  out[i * 3 + 1] = ok ? sy / l : 0.0f;
  out[i * 3 + 2] = ok ? sz / l : 0.0f;
}

// ---- b. connected components: lock-free union-find ---------------------------------------------------------------------
// parent[x] <= x always, and parent[x] is a vertex of x's component.  A root (parent[x] == x) is only ever hooked under a
// SMALLER root, by one compare-and-swap; a hooked vertex never becomes a root again, and its link is only ever lowered, by
// atomicMin, to one of its ancestors (path halving: without it a wall's scanline order builds chains thousands long).  So
// every chain descends strictly, the last root standing is the component's minimum whatever the order of the hooks and of
// the halvings, and every loop below is bounded: a step either ends it or lowers an index that is >= 0.

__device__ __forceinline__ int32_t load_parent(const int32_t* parent, int32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x) {
  int32_t p = load_parent(parent, x);
  while (p < x) {                      // strictly descending; a root has p == x
    const int32_t g = load_parent(parent, p);
    if (g < p) atomicMin(parent + x, g);                           // x is hooked already: the compare-and-swap never sees it
    x = p;
    p = g;
  }
  return x;
}

__device__ void unite(int32_t* parent, int32_t a, int32_t b) {
  a = find_root(parent, a);
  b = find_root(parent, b);
  while (a != b) {
    if (a < b) { const int32_t t = a; a = b; b = t; }            // a is the larger root
    const int32_t old = atomicCAS(parent + a, a, b);
    if (old == a) return;                                        // hooked
    a = find_root(parent, old);                                  // somebody hooked a first, under old < a: a + b fell
    b = find_root(parent, b);
  }
}

__global__ void __launch_bounds__(NT) identity_kernel(int32_t* __restrict__ parent, int64_t V) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i < V) parent[i] = (int32_t)i;
}

__global__ void __launch_bounds__(NT) union_kernel(const int32_t* __restrict__ f, int64_t F, int32_t* parent) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= F) return;
  const int32_t a = f[i * 3], b = f[i * 3 + 1], c = f[i * 3 + 2];
  unite(parent, a, b);
  unite(parent, b, c);
}

// after the unions are complete (a launch of its own): no root changes any more, links are still halved
__global__ void __launch_bounds__(NT) flatten_kernel(int32_t* parent, int64_t V, int32_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i < V) labels[i] = find_root(parent, (int32_t)i);
}

// ---- c. small components and compaction ------------------------------------------------------------------------------

__global__ void __launch_bounds__(NT) component_faces_kernel(const int32_t* __restrict__ f, int64_t F,
                                                             const int32_t* __restrict__ labels, int32_t* counts) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i < F) atomicAdd(counts + labels[f[i * 3]], 1);             // integers: the order does not matter
}

__global__ void __launch_bounds__(NT) keep_faces_kernel(const int32_t* __restrict__ f, int64_t F, const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ counts, int32_t min_faces,
                                                        int32_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i < F) keep[i] = counts[labels[f[i * 3]]] >= min_faces ? 1 : 0;
}

__global__ void __launch_bounds__(NT) mark_vertices_kernel(const int32_t* __restrict__ f, int64_t F, const int32_t* __restrict__ keep,
                                                           int32_t* used) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= F || (keep && !keep[i])) return;
  used[f[i * 3]] = 1;                                             // every writer writes 1
  used[f[i * 3 + 1]] = 1;
  used[f[i * 3 + 2]] = 1;
}

__global__ void __launch_bounds__(NT) compact_vertices_kernel(const float* __restrict__ v, const float* __restrict__ c, int64_t V,
                                                              const int32_t* __restrict__ used, const int64_t* __restrict__ offsets,
                                                              float* __restrict__ out_v, float* __restrict__ out_c,
                                                              int32_t* __restrict__ vmap) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= V) return;
  if (!used[i]) { vmap[i] = -1; return; }
  const int64_t j = offsets[i];
  vmap[i] = (int32_t)j;
  for (int k = 0; k < 3; ++k) {
    out_v[j * 3 + k] = v[i * 3 + k];
    out_c[j * 3 + k] = c[i * 3 + k];
  }
}

__global__ void __launch_bounds__(NT) compact_faces_kernel(const int32_t* __restrict__ f, int64_t F, const int32_t* __restrict__ keep,
                                                           const int64_t* __restrict__ offsets, const int32_t* __restrict__ vmap,
                                                           int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= F || (keep && !keep[i])) return;
  const int64_t j = keep ? offsets[i] : i;
  for (int k = 0; k < 3; ++k) {
    const int32_t x = f[i * 3 + k];
    out[j * 3 + k] = vmap ? vmap[x] : x;
  }
}

// ---- d. vertex clustering --------------------------------------------------------------------------------------------

// c = (int) floorf((p - origin) / cell) per axis; err[0] = 1 when a vertex lies below origin (or is NaN), or past MAX_CELLS
__global__ void __launch_bounds__(NT) cluster_cells_kernel(const float* __restrict__ v, int64_t V, float ox, float oy, float oz,
                                                           float cell, int32_t* __restrict__ cells, int32_t* err) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= V) return;
  const float o[3] = {ox, oy, oz};
  for (int k = 0; k < 3; ++k) {
    const float d = v[i * 3 + k] - o[k];
    const float q = floorf(d / cell);
    const bool ok = d >= 0.0f && q < (float)RTGS_MESH_MAX_CELLS;
    if (!ok) err[0] = 1;
    cells[i * 3 + k] = ok ? (int32_t)q : 0;
  }
}

// one thread per occupied cell: members order[start[s] .. start[s + 1]) in ascending vertex index, summed in float64
__global__ void __launch_bounds__(NT) cluster_means_kernel(const float* __restrict__ v, const float* __restrict__ c,
                                                           const int64_t* __restrict__ order, const int64_t* __restrict__ start,
                                                           int64_t S, float* __restrict__ out_v, float* __restrict__ out_c) {
  const int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (s >= S) return;
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t begin = start[s], end = start[s + 1];
  for (int64_t j = begin; j < end; ++j) {
    const int64_t i = order[j];
    for (int k = 0; k < 3; ++k) {
      a[k] = a[k] + (double)v[i * 3 + k];
      a[3 + k] = a[3 + k] + (double)c[i * 3 + k];
    }
  }
  const double n = (double)(end - begin);
  for (int k = 0; k < 3; ++k) {
    out_v[s * 3 + k] = (float)(a[k] / n);
    out_c[s * 3 + k] = (float)(a[3 + k] / n);
  }
}

// faces in cluster indices, rotated so the smallest comes first (winding kept); valid = 0 when two corners share a cell
__global__ void __launch_bounds__(NT) cluster_faces_kernel(const int32_t* __restrict__ f, int64_t F, const int32_t* __restrict__ cluster,
                                                           int32_t* __restrict__ out, int32_t* __restrict__ valid) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= F) return;
  int32_t a = cluster[f[i * 3]], b = cluster[f[i * 3 + 1]], c = cluster[f[i * 3 + 2]];
  valid[i] = (a != b && b != c && a != c) ? 1 : 0;
  if (b < a && b < c) { const int32_t t = a; a = b; b = c; c = t; }
  else if (c < a && c < b) { const int32_t t = a; a = c; c = b; b = t; }
  out[i * 3] = a;
  out[i * 3 + 1] = b;
  out[i * 3 + 2] = c;
}

// ids: the valid faces sorted stably by (a, b, c); the first of every run of identical faces is the first in original order
__global__ void __launch_bounds__(NT) mark_first_kernel(const int32_t* __restrict__ f, const int64_t* __restrict__ ids, int64_t n,
                                                        int32_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int64_t x = ids[i];
  bool first = i == 0;
  if (!first) {
    const int64_t y = ids[i - 1];
    first = f[x * 3] != f[y * 3] || f[x * 3 + 1] != f[y * 3 + 1] || f[x * 3 + 2] != f[y * 3 + 2];
  }
  keep[x] = first ? 1 : 0;
}

}  // namespace rtgs_mesh

#define RTGS_MESH_LAUNCH(n, kernel, ...)                                                              \
  do {                                                                                                \
    unsigned blocks_;                                                                                 \
    if (!grid_for((n), &blocks_)) return -1;                                                          \
    hipLaunchKernelGGL(kernel, dim3(blocks_), dim3(NT), 0, (hipStream_t)stream, __VA_ARGS__);         \
    if (hipGetLastError() != hipSuccess) return -2;                                                   \
  } while (0)

extern "C" {

using namespace rtgs_mesh;

static bool bad_counts(int64_t V, int64_t F) { return V < 0 || F < 0 || V > RTGS_MESH_MAX_ELEMENTS || F > RTGS_MESH_MAX_ELEMENTS; }

int rtgs_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t V, int64_t F, const int64_t* order,
                             const int64_t* start, float* normals, void* stream) {
  if (bad_counts(V, F)) return -1;
  if (V == 0) return 0;
  if (!vertices || !start || !normals || (F > 0 && (!faces || !order))) return -1;
  RTGS_MESH_LAUNCH(V, normals_kernel, vertices, faces, order, start, V, normals);
  return 0;
}

int rtgs_mesh_component_labels(const int32_t* faces, int64_t F, int64_t V, int32_t* parent, int32_t* labels, void* stream) {
  if (bad_counts(V, F)) return -1;
  if (V == 0) return 0;
  if (!parent || !labels || parent == labels || (F > 0 && !faces)) return -1;
  RTGS_MESH_LAUNCH(V, identity_kernel, parent, V);
  if (F > 0) RTGS_MESH_LAUNCH(F, union_kernel, faces, F, parent);
  RTGS_MESH_LAUNCH(V, flatten_kernel, parent, V, labels);
  return 0;
}

int rtgs_mesh_component_faces(const int32_t* faces, int64_t F, const int32_t* labels, int32_t* counts, void* stream) {
  if (bad_counts(0, F)) return -1;
  if (F == 0) return 0;
  if (!faces || !labels || !counts) return -1;
  RTGS_MESH_LAUNCH(F, component_faces_kernel, faces, F, labels, counts);
  return 0;
}

int rtgs_mesh_keep_faces(const int32_t* faces, int64_t F, const int32_t* labels, const int32_t* counts, int32_t min_faces,
                         int32_t* keep, void* stream) {
  if (bad_counts(0, F)) return -1;
  if (F == 0) return 0;
  if (!faces || !labels || !counts || !keep) return -1;
  RTGS_MESH_LAUNCH(F, keep_faces_kernel, faces, F, labels, counts, min_faces, keep);
  return 0;
}

int rtgs_mesh_mark_vertices(const int32_t* faces, int64_t F, const int32_t* keep, int32_t* used, void* stream) {
  if (bad_counts(0, F)) return -1;
  if (F == 0) return 0;
  if (!faces || !used) return -1;
  RTGS_MESH_LAUNCH(F, mark_vertices_kernel, faces, F, keep, used);
  return 0;
}

int rtgs_mesh_compact_vertices(const float* vertices, const float* colors, int64_t V, const int32_t* used, const int64_t* offsets,
                               float* out_vertices, float* out_colors, int32_t* vmap, void* stream) {
  if (bad_counts(V, 0)) return -1;
  if (V == 0) return 0;
  if (!vertices || !colors || !used || !offsets || !out_vertices || !out_colors || !vmap) return -1;
  RTGS_MESH_LAUNCH(V, compact_vertices_kernel, vertices, colors, V, used, offsets, out_vertices, out_colors, vmap);
  return 0;
}

int rtgs_mesh_compact_faces(const int32_t* faces, int64_t F, const int32_t* keep, const int64_t* offsets, const int32_t* vmap,
                            int32_t* out_faces, void* stream) {
  if (bad_counts(0, F)) return -1;
  if (F == 0) return 0;
  if (!faces || !out_faces || (keep && !offsets)) return -1;
  RTGS_MESH_LAUNCH(F, compact_faces_kernel, faces, F, keep, offsets, vmap, out_faces);
  return 0;
}

int rtgs_mesh_cluster_cells(const float* vertices, int64_t V, const float* origin3_host, float cell, int32_t* cells, int32_t* err,
                            void* stream) {
  if (bad_counts(V, 0) || !origin3_host || !(cell > 0.0f)) return -1;
  if (V == 0) return 0;
  if (!vertices || !cells || !err) return -1;
  RTGS_MESH_LAUNCH(V, cluster_cells_kernel, vertices, V, origin3_host[0], origin3_host[1], origin3_host[2], cell, cells, err);
  return 0;
}

int rtgs_mesh_cluster_means(const float* vertices, const float* colors, const int64_t* order, const int64_t* start, int64_t S,
                            float* out_vertices, float* out_colors, void* stream) {
  if (bad_counts(S, 0)) return -1;
  if (S == 0) return 0;
  if (!vertices || !colors || !order || !start || !out_vertices || !out_colors) return -1;
  RTGS_MESH_LAUNCH(S, cluster_means_kernel, vertices, colors, order, start, S, out_vertices, out_colors);
  return 0;
}

int rtgs_mesh_cluster_faces(const int32_t* faces, int64_t F, const int32_t* cluster, int32_t* out_faces, int32_t* valid,
                            void* stream) {
  if (bad_counts(0, F)) return -1;
  if (F == 0) return 0;
  if (!faces || !cluster || !out_faces || !valid) return -1;
  RTGS_MESH_LAUNCH(F, cluster_faces_kernel, faces, F, cluster, out_faces, valid);
  return 0;
}

int rtgs_mesh_mark_first(const int32_t* faces, const int64_t* ids, int64_t n, int32_t* keep, void* stream) {
  if (bad_counts(0, n)) return -1;
  if (n == 0) return 0;
  if (!faces || !ids || !keep) return -1;
  RTGS_MESH_LAUNCH(n, mark_first_kernel, faces, ids, n, keep);
  return 0;
}

}  // extern "C"
