// gfx950 kernels + C ABI of the mesh decimation (include/rtgs_slam.h, "mesh decimation"): parallel quadric-error HALF-EDGE
// collapse in rounds, on the indexed triangle mesh (vertices [V][3] float32, faces [F][3] int32) the other mesh operations
// leave on the device.  A collapse u -> v removes vertex u and moves nothing, so the only float work is the cost and the
// flip test: float64, one rounded operation per step, in the order tests/mesh_decimate_reference.py writes out in numpy; the
// kernels match it bit for bit.  Built with -ffp-contract=off (Makefile EXTRA_mesh_decimate).
//
// Nothing here adds floats atomically.  A vertex's quadric is summed by ONE thread over its corners in ascending corner
// index; an applied collapse adds Q[u] to Q[v] and at most one u reaches a given v per round.  The independent set is an
// integer atomicMin of ranks: the minimum commutes, so the selection does not depend on thread order.  Every kernel is a
// dependent gather over a vertex's corner list: latency-bound, sized by V and F, not by bytes.
//
// Index range: the caller guarantees 0 <= faces[i] < V (rtg_slam_amd/mesh_ops.py checks it once); the kernels trust it.
// Element indices are 64-bit where 3 F can pass 2^31.
#include "../../include/rtgs_slam.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtgs_decimate {

constexpr int NT = 256;
constexpr int PT = 64;                                   // the propose kernel: one wave per block, see s_x below
constexpr int MAXV = RTGS_MESH_DECIMATE_MAX_VALENCE;
constexpr int MINV = RTGS_MESH_DECIMATE_MIN_VALENCE;
constexpr int NQ = 11;                                   // 10 upper entries of the symmetric 4x4, then the weight

inline bool grid_for(int64_t n, int threads, unsigned* blocks) {
  const int64_t b = (n + threads - 1) / threads;
  if (b > 0x7fffffffLL) return false;
  *blocks = (unsigned)b;
  return true;
}

struct d3 { double x, y, z; };

__device__ __forceinline__ d3 load3(const float* __restrict__ v, int64_t i) {
  return {(double)v[i * 3], (double)v[i * 3 + 1], (double)v[i * 3 + 2]};
}
__device__ __forceinline__ d3 sub(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// every component two rounded products and a rounded difference
__device__ __forceinline__ d3 cross(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(d3 a, d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// the corner o = 3 f + k of a vertex -> the two other corners of its face, in the face's cyclic order
__device__ __forceinline__ void others(const int32_t* __restrict__ f, int64_t o, int32_t* x, int32_t* y) {
  const int64_t g = o / 3;
  const int k = (int)(o - g * 3);
  *x = f[g * 3 + (k + 1) % 3];
  *y = f[g * 3 + (k + 2) % 3];
}

// ---- a. vertex quadrics --------------------------------------------------------------------------------------------------

// one thread per vertex: Q[v] = 0 + the plane quadric of every corner's face, in ascending corner index.  The face is taken
// in its STORED corner order, so its three corners add the same 11 numbers.
__global__ void __launch_bounds__(NT) quadrics_kernel(const float* __restrict__ v, const int32_t* __restrict__ f,
                                                      const int64_t* __restrict__ order, const int64_t* __restrict__ start,
                                                      int64_t V, double* __restrict__ Q) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= V) return;
  double q[NQ];
  for (int e = 0; e < NQ; ++e) q[e] = 0.0;
  const int64_t end = start[i + 1];
  for (int64_t j = start[i]; j < end; ++j) {
    const int64_t g = order[j] / 3;
    const d3 pa = load3(v, f[g * 3]), pb = load3(v, f[g * 3 + 1]), pc = load3(v, f[g * 3 + 2]);
    const d3 n = cross(sub(pb, pa), sub(pc, pa));
    const double l = sqrt(dot(n, n));
    if (!(l > 0.0)) continue;                                      // an area-less face (or NaN) contributes nothing
    const double pl[4] = {n.x / l, n.y / l, n.z / l, -dot(d3{n.x / l, n.y / l, n.z / l}, pa)};
    const double w = l / 2.0;
    int e = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = r; c < 4; ++c, ++e) q[e] = q[e] + w * (pl[r] * pl[c]);
    q[10] = q[10] + w;
  }
  for (int e = 0; e < NQ; ++e) Q[i * NQ + e] = q[e];
}

// ---- b. locks ---------------------------------------------------------------------------------------------------------------

// the three undirected edges (a,b) (b,c) (c,a) of a face as keys min V + max: past 2^31 from V = 46341 on
__global__ void __launch_bounds__(NT) edge_keys_kernel(const int32_t* __restrict__ f, int64_t F, int64_t V, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= F) return;
  const int64_t a = f[i * 3], b = f[i * 3 + 1], c = f[i * 3 + 2];
  keys[i * 3] = (a < b ? a : b) * V + (a < b ? b : a);
  keys[i * 3 + 1] = (b < c ? b : c) * V + (b < c ? c : b);
  keys[i * 3 + 2] = (c < a ? c : a) * V + (c < a ? a : c);
}

// one thread per run of equal keys: an edge without exactly 2 faces (boundary or non-manifold) locks both of its vertices
__global__ void __launch_bounds__(NT) locks_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ counts, int64_t n,
                                                   int64_t V, int32_t* locked) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n || counts[i] == 2) return;
  const int64_t lo = keys[i] / V;
  locked[lo] = 1;                                                  // every writer writes 1
  locked[keys[i] - lo * V] = 1;
}

// ---- c. proposals ----------------------------------------------------------------------------------------------------------

// p^T q p with p = (x, y, z, 1), in the order the reference writes out; negative (rounding) and NaN become 0
__device__ __forceinline__ double quadric_cost(const double* q, d3 p) {
  const double r0 = ((q[0] * p.x + q[1] * p.y) + q[2] * p.z) + q[3];
  const double r1 = ((q[1] * p.x + q[4] * p.y) + q[5] * p.z) + q[6];
  const double r2 = ((q[2] * p.x + q[5] * p.y) + q[7] * p.z) + q[8];
  const double r3 = ((q[3] * p.x + q[6] * p.y) + q[8] * p.z) + q[9];
  const double c = ((r0 * p.x + r1 * p.y) + r2 * p.z) + r3;
  return c > 0.0 ? c : 0.0;
}

// One thread per vertex u.  A removable u (not locked, MINV..MAXV faces) tests every neighbour v: link condition, no flip,
// cost, error bound; it proposes the valid v with the smallest (cost, v).  prop[u] = v or -1, cost[u] = that cost.
// The faces of u (their two other corners) and its ring are indexed at run time, so as per-thread arrays they would live in
// scratch memory.  They live in LDS instead, slot-major (slot * PT + thread: consecutive lanes, consecutive banks):
// 3 arrays x 32 slots x 64 threads x 4 B = 24 KB per block of one wave, six blocks per CU.  Each thread touches only its own
// column, so no barrier is needed.
__global__ void __launch_bounds__(PT) propose_kernel(const float* __restrict__ v, const int32_t* __restrict__ f,
                                                     const int64_t* __restrict__ order, const int64_t* __restrict__ start,
                                                     const int32_t* __restrict__ locked, const double* __restrict__ Q, int64_t V,
                                                     double max_error, int32_t* __restrict__ prop, double* __restrict__ cost_out) {
  __shared__ int32_t s_x[MAXV * PT], s_y[MAXV * PT], s_ring[MAXV * PT];
  const int t = threadIdx.x;
  const int64_t u = (int64_t)blockIdx.x * PT + t;
  if (u >= V) return;
  int32_t best = -1;
  double best_cost = 0.0;
  const int64_t begin = start[u];
  const int64_t n64 = start[u + 1] - begin;
  bool removable = !locked[u] && n64 >= MINV && n64 <= MAXV;
  const int n = removable ? (int)n64 : 0;
  int nr = 0;
  for (int i = 0; i < n; ++i) {
    int32_t xy[2];
    others(f, order[begin + i], &xy[0], &xy[1]);
    s_x[i * PT + t] = xy[0];
    s_y[i * PT + t] = xy[1];
    for (int k = 0; k < 2; ++k) {
      bool seen = false;
      for (int r = 0; r < nr; ++r) seen = seen || s_ring[r * PT + t] == xy[k];
      if (seen) continue;
      // every edge of an unlocked vertex has 2 faces, so it has as many neighbours as faces; a mesh that breaks this is refused
      if (nr == MAXV) { removable = false; break; }
      s_ring[nr * PT + t] = xy[k];
      ++nr;
    }
  }
  if (removable) {
    const d3 pu = load3(v, u);
    double qu[NQ];
    for (int e = 0; e < NQ; ++e) qu[e] = Q[u * NQ + e];
    for (int c = 0; c < nr; ++c) {
      const int32_t w = s_ring[c * PT + t];
      // (a) link condition: N(u) and N(w) share exactly 2 vertices.  N(w) may be long (no valence bound on a target).
      uint32_t shared = 0;
      const int64_t wend = start[(int64_t)w + 1];
      for (int64_t j = start[w]; j < wend; ++j) {
        int32_t a, b;
        others(f, order[j], &a, &b);
        for (int r = 0; r < nr; ++r) {
          const int32_t x = s_ring[r * PT + t];
          if (x == a || x == b) shared |= 1u << r;
        }
      }
      if (__popc(shared) != 2) continue;
      // (b) no flip: every face (u, x, y) of u without w keeps a strictly positive dot of its cross products; a w that stands
      // exactly where u stands changes no face and passes whatever their areas (it welds a duplicate vertex)
      const d3 pw = load3(v, w);
      bool ok = true;
      const bool same = pu.x == pw.x && pu.y == pw.y && pu.z == pw.z;
      for (int i = 0; i < n && ok && !same; ++i) {
        const int32_t x = s_x[i * PT + t], y = s_y[i * PT + t];
        if (x == w || y == w) continue;
        const d3 px = load3(v, x), py = load3(v, y);
        const d3 before = cross(sub(px, pu), sub(py, pu));
        const d3 after = cross(sub(px, pw), sub(py, pw));
        ok = dot(before, after) > 0.0;
      }
      if (!ok) continue;
      // (c) the cost of standing at w for both quadrics, (d) the bound on it
      double q[NQ];
      for (int e = 0; e < NQ; ++e) q[e] = qu[e] + Q[(int64_t)w * NQ + e];
      const double cost = quadric_cost(q, pw);
      if (max_error > 0.0 && !(sqrt(cost / q[10]) <= max_error)) continue;
      if (best < 0 || cost < best_cost || (cost == best_cost && w < best)) {
        best = w;
        best_cost = cost;
      }
    }
  }
  prop[u] = best;
  cost_out[u] = best_cost;
}

// ---- d. independent set ----------------------------------------------------------------------------------------------------

// fn(x) for every vertex of N[u] + N[w], the closed neighbourhoods (some more than once)
template <class Fn>
__device__ __forceinline__ void walk_closed(const int32_t* __restrict__ f, const int64_t* __restrict__ order,
                                            const int64_t* __restrict__ start, int32_t u, int32_t w, Fn fn) {
  const int32_t ends[2] = {u, w};
  for (int s = 0; s < 2; ++s) {
    const int64_t c = ends[s];
    fn(ends[s]);
    const int64_t end = start[c + 1];
    for (int64_t j = start[c]; j < end; ++j) {
      int32_t a, b;
      others(f, order[j], &a, &b);
      fn(a);
      fn(b);
    }
  }
}

// one thread per participant, rank r: claim[x] = min(claim[x], r) over N[u] + N[v]
__global__ void __launch_bounds__(NT) claim_kernel(const int32_t* __restrict__ f, const int64_t* __restrict__ order,
                                                   const int64_t* __restrict__ start, const int64_t* __restrict__ ranked,
                                                   const int32_t* __restrict__ prop, int64_t P, int32_t* claim) {
  const int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (r >= P) return;
  const int32_t u = (int32_t)ranked[r];
  walk_closed(f, order, start, u, prop[u], [&](int32_t x) { atomicMin(claim + x, (int32_t)r); });
}

// after the claims are complete (a launch of its own): selected when it holds all of them
__global__ void __launch_bounds__(NT) select_kernel(const int32_t* __restrict__ f, const int64_t* __restrict__ order,
                                                    const int64_t* __restrict__ start, const int64_t* __restrict__ ranked,
                                                    const int32_t* __restrict__ prop, int64_t P, const int32_t* __restrict__ claim,
                                                    int32_t* __restrict__ selected) {
  const int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (r >= P) return;
  const int32_t u = (int32_t)ranked[r];
  bool all = true;
  walk_closed(f, order, start, u, prop[u], [&](int32_t x) { all = all && claim[x] == (int32_t)r; });
  selected[r] = all ? 1 : 0;
}

// ---- e. apply ---------------------------------------------------------------------------------------------------------------

// one thread per participant: an applied collapse u -> v writes remap[u] = v and Q[v] = Q[v] + Q[u].  Applied collapses have
// disjoint N[u] + N[v]: no two write one v, and no u is another's v.
__global__ void __launch_bounds__(NT) apply_kernel(const int64_t* __restrict__ ranked, const int32_t* __restrict__ prop,
                                                   const int32_t* __restrict__ applied, int64_t P, int32_t* __restrict__ remap,
                                                   double* Q) {
  const int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (r >= P || !applied[r]) return;
  const int64_t u = ranked[r];
  const int64_t w = prop[u];
  remap[u] = (int32_t)w;
  for (int e = 0; e < NQ; ++e) Q[w * NQ + e] = Q[w * NQ + e] + Q[u * NQ + e];
}

// keep[f] = 0 for a face that has two equal corners once they pass through remap
__global__ void __launch_bounds__(NT) reindex_kernel(const int32_t* __restrict__ f, int64_t F, const int32_t* __restrict__ remap,
                                                     int32_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= F) return;
  const int32_t a = remap[f[i * 3]], b = remap[f[i * 3 + 1]], c = remap[f[i * 3 + 2]];
  keep[i] = (a != b && b != c && a != c) ? 1 : 0;
}

}  // namespace rtgs_decimate

#define RTGS_DECIMATE_LAUNCH(n, threads, kernel, ...)                                                  \
  do {                                                                                                \
    unsigned blocks_;                                                                                 \
    if (!grid_for((n), (threads), &blocks_)) return -1;                                               \
    hipLaunchKernelGGL(kernel, dim3(blocks_), dim3(threads), 0, (hipStream_t)stream, __VA_ARGS__);    \
    if (hipGetLastError() != hipSuccess) return -2;                                                   \
  } while (0)

extern "C" {

using namespace rtgs_decimate;

static bool bad_counts(int64_t V, int64_t F) { return V < 0 || F < 0 || V > RTGS_MESH_MAX_ELEMENTS || F > RTGS_MESH_MAX_ELEMENTS; }

int rtgs_mesh_decimate_quadrics(const float* vertices, const int32_t* faces, int64_t V, int64_t F, const int64_t* order,
                                const int64_t* start, double* quadrics, void* stream) {
  if (bad_counts(V, F)) return -1;
  if (V == 0) return 0;
  if (!vertices || !start || !quadrics || (F > 0 && (!faces || !order))) return -1;
  RTGS_DECIMATE_LAUNCH(V, NT, quadrics_kernel, vertices, faces, order, start, V, quadrics);
  return 0;
}

int rtgs_mesh_decimate_edge_keys(const int32_t* faces, int64_t F, int64_t V, int64_t* keys, void* stream) {
  if (bad_counts(V, F)) return -1;
  if (F == 0) return 0;
  if (!faces || !keys || V == 0) return -1;
  RTGS_DECIMATE_LAUNCH(F, NT, edge_keys_kernel, faces, F, V, keys);
  return 0;
}

int rtgs_mesh_decimate_locks(const int64_t* keys, const int64_t* counts, int64_t n, int64_t V, int32_t* locked, void* stream) {
  if (bad_counts(V, 0) || n < 0 || n > 3 * RTGS_MESH_MAX_ELEMENTS) return -1;
  if (n == 0) return 0;
  if (!keys || !counts || !locked || V == 0) return -1;
  RTGS_DECIMATE_LAUNCH(n, NT, locks_kernel, keys, counts, n, V, locked);
  return 0;
}

int rtgs_mesh_decimate_propose(const float* vertices, const int32_t* faces, int64_t V, int64_t F, const int64_t* order,
                               const int64_t* start, const int32_t* locked, const double* quadrics, double max_error,
                               int32_t* proposal, double* cost, void* stream) {
  if (bad_counts(V, F) || max_error != max_error) return -1;
  if (V == 0) return 0;
  if (!vertices || !start || !locked || !quadrics || !proposal || !cost || (F > 0 && (!faces || !order))) return -1;
  RTGS_DECIMATE_LAUNCH(V, PT, propose_kernel, vertices, faces, order, start, locked, quadrics, V, max_error, proposal, cost);
  return 0;
}

int rtgs_mesh_decimate_claim(const int32_t* faces, const int64_t* order, const int64_t* start, const int64_t* ranked,
                             const int32_t* proposal, int64_t P, int32_t* claim, void* stream) {
  if (bad_counts(P, 0)) return -1;
  if (P == 0) return 0;
  if (!faces || !order || !start || !ranked || !proposal || !claim) return -1;
  RTGS_DECIMATE_LAUNCH(P, NT, claim_kernel, faces, order, start, ranked, proposal, P, claim);
  return 0;
}

int rtgs_mesh_decimate_select(const int32_t* faces, const int64_t* order, const int64_t* start, const int64_t* ranked,
                              const int32_t* proposal, int64_t P, const int32_t* claim, int32_t* selected, void* stream) {
  if (bad_counts(P, 0)) return -1;
  if (P == 0) return 0;
  if (!faces || !order || !start || !ranked || !proposal || !claim || !selected) return -1;
  RTGS_DECIMATE_LAUNCH(P, NT, select_kernel, faces, order, start, ranked, proposal, P, claim, selected);
  return 0;
}

int rtgs_mesh_decimate_apply(const int64_t* ranked, const int32_t* proposal, const int32_t* applied, int64_t P, int32_t* remap,
                             double* quadrics, void* stream) {
  if (bad_counts(P, 0)) return -1;
  if (P == 0) return 0;
  if (!ranked || !proposal || !applied || !remap || !quadrics) return -1;
  RTGS_DECIMATE_LAUNCH(P, NT, apply_kernel, ranked, proposal, applied, P, remap, quadrics);
  return 0;
}

int rtgs_mesh_decimate_reindex(const int32_t* faces, int64_t F, const int32_t* remap, int32_t* keep, void* stream) {
  if (bad_counts(0, F)) return -1;
  if (F == 0) return 0;
  if (!faces || !remap || !keep) return -1;
  RTGS_DECIMATE_LAUNCH(F, NT, reindex_kernel, faces, F, remap, keep);
  return 0;
}

}  // extern "C"
