// gfx950 kernels + C ABI of the point-to-mesh distance (include/rtgs_slam.h, "mesh distance"): for every query point the exact
// float32 squared distance to the nearest triangle of an indexed mesh, and that triangle's index.  No counterpart in the
// reference; tests/mesh_distance_reference.py restates it in numpy - a brute force over ALL faces - and is the definition, matched
// bit for bit.  Built with -ffp-contract=off (Makefile EXTRA_mesh_distance): every float step of pair_d2 below is one correctly
// rounded operation, in the definition's order.
//
// The index is a uniform grid (origin, cell, dims chosen by the host) with a list of face indices per cell, above it blocks of
// 4 x 4 x 4 cells with an occupied flag, and above those super blocks of 4 x 4 x 4 blocks with one: a point metres from any
// surface walks rings of 16-cell super blocks, not of cells.  Launches, all on the caller's stream:
// count      faces<false>: one thread per face.  face_cells() gives the face's cell box (its AABB, inflated) and its plane; the
//            face is registered in every cell of the box that the inflated plane test (crossed()) passes.  A box of at most
//            large_max cells is walked by its thread, a larger one is appended to a queue: one integer atomic add per wave
//            (ballot, prefix count).  large<false>: a fixed grid of waves strides over the queue, one face per wave, the 64
//            lanes over the box.  Both add 1 to counts[cell] with an integer atomic.
// (host)     the exclusive scan of counts -> start [cells + 1]; its last value, the number of entries, is the one host read.
// fill       faces<true> and large<true>: the same walk through the same two device functions, so the same cells; an entry
//            goes to entries[start[cell] + atomicAdd(cursor[cell], 1)].  The order inside a cell is not deterministic and
//            need not be: the query keeps the lexicographic minimum of (d2, face), which is order-free.  The queue of the
//            count pass is reused.
// blocks     one thread per block: occupied when one of its cells has an entry; then one thread per super block likewise.
// query      one thread per point (through `order` when the caller sorted the points by cell): Chebyshev rings of super blocks
//            around the point's clamped cell, empty ones skipped, then per super block, per block and per cell a lower bound of
//            the distance from the integer cell offsets; pair_d2 for the entries of the cells that pass.  See "Why the walk
//            may stop".  query_bounded is the same walk under a caller's radius (step 5), a kernel of its own.
// keys       the clamped cell of every point as one int64, for the caller's sort.
// normals    the unit normal of face[i].
//
// Why the walk may stop ("mesh distance", has the derivation).  u = 2^-24.  M = the largest |coordinate| of the mesh,
// P = the largest |coordinate| of the point.
//  1 Every candidate of pair_d2 is |p - y|^2 for a point y = a + s ab + t ac of the face with (s, t) in the triangle WHATEVER s
//    and t came out as, evaluated with a componentwise error of at most u (3 P + 19 M) and a relative error of 3 u in the dot.
//    So sqrt(pair_d2) >= D - eta, D the true distance, eta = 2^-20 (P + 4 M) (about twice what the sum of the terms needs).
//  2 (x - origin) * inv_cell is off by at most 3 u 2^16 < 1/64 of a cell (dims <= 65536 per axis); boxes are inflated by 1/16.
//    The plane test keeps a cell when |n . (centre - a)| <= 0.5625 cell |n|_1 + 2^-18 |ab|_1 |ac|_1 (|centre - a|_1 + cell + M):
//    the second term is twice the rounding of n, of the centre and of the dot, so a needle's noisy normal keeps every cell.
//    Hence every true point of a face lies in a cell the face is registered in.
//  3 A cell whose index differs from the point's clamped cell by k on some axis is at least (k - 1 - 1/32) cell away on that
//    axis (projection onto the grid's box does not expand distances); the code uses (k - 1 - 1/16) cell, and the sum of the
//    squares of the three axes: a lower bound lb2 <= D^2 for every face registered only in such cells.
//  4 thr = (sqrt(best) + eta) (1 + 2^-20), thr2 = thr thr (1 + 2^-20) are rounded up past their exact values.  A ring, super block, block or
//    cell is skipped only when lb2 > thr2: then D > sqrt(best) + eta, and by 1 the face's pair_d2 is > best.  A face whose
//    pair_d2 is <= best is therefore never skipped: the bits and the lowest-index tie rule of the brute force are kept.
//  5 The bounded query (rtgs_mesh_distance_query_bounded: "the nearest face within max_d2, or nothing") is the same walk with
//    two changes: thr2 starts at cap_thr2, from cap_thr = (sqrt(max_d2) + eta) (1 + 2^-20), cap_thr2 = cap_thr cap_thr
//    (1 + 2^-20), and a candidate is offered only when pair_d2 <= max_d2.  The chain of 4 is monotone in best, so every later
//    thr2 is <= cap_thr2.  A face with pair_d2 <= max_d2 has by 1 a true distance D <= sqrt(max_d2) + eta, and by 3 every cell
//    it is registered in has lb2 <= D^2 <= cap_thr2: the cap does not skip it, and a later thr2 comes from a best <= max_d2, to
//    which 4 applies unchanged.  All faces with pair_d2 <= max_d2 therefore compete exactly as in the unbounded walk, lowest
//    index first among equals; the faces beyond cannot win and need not be seen.  A point metres from any surface finds every
//    bound of ring 0 and ring 1 above the cap and is done.  The unbounded query is its own instantiation (BOUNDED = false:
//    no cap, no test), not the bounded one with max_d2 = inf.
//
// Index range: the caller guarantees 0 <= faces[i] < V, finite vertices with |coordinate| <= 2^20, and that the grid holds the
// mesh with half a cell to spare (mesh_ops.MeshDistance checks all three once).  Element indices are 64-bit.
#include "../../include/rtgs_slam.h"
#include "mesh_face_normal.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace rtgs_mesh_distance_k {

constexpr int NT = 256;
constexpr int WAVE = 64;
constexpr int LARGE_BLOCKS = 2048;                         // x 4 waves: the fixed grid of the large-face kernels
constexpr int BLOCK = RTGS_MESH_DISTANCE_BLOCK;            // cells per block edge
constexpr int SUPER = RTGS_MESH_DISTANCE_SUPER;            // blocks per super block edge
constexpr int MAX_DIM = RTGS_MESH_DISTANCE_MAX_DIM;
constexpr float BOX_SLACK = 0.0625f;                       // cells
constexpr float UP = 1.0f + 9.5367431640625e-07f;          // 1 + 2^-20
constexpr float ETA = 9.5367431640625e-07f;                // 2^-20
constexpr float PLANE_HALF = 0.5625f;                      // cells
constexpr float PLANE_ABS = 3.814697265625e-06f;           // 2^-18

struct Grid {
  float ox, oy, oz, h, inv_h;
  int nx, ny, nz;              // cells
  int bx, by, bz;              // blocks: ceil(n / BLOCK)
  int sx, sy, sz;              // super blocks: ceil(b / SUPER)
  float vmax;                  // M
};

struct FaceCells {
  int x0, y0, z0, wx, wy, wz;  // the cell box: x0 .. x0 + wx - 1, ...
  float ax, ay, az, nx, ny, nz;
  float half;                  // PLANE_HALF h |n|_1
  float lablac;                // PLANE_ABS |ab|_1 |ac|_1
};

inline bool grid_for(int64_t n, unsigned* blocks) {
  const int64_t b = (n + NT - 1) / NT;
  if (b > 0x7fffffffLL) return false;
  *blocks = (unsigned)b;
  return true;
}

__host__ __device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__host__ __device__ __forceinline__ int iabs(int a) { return a < 0 ? -a : a; }

__host__ __device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__host__ __device__ __forceinline__ float clamp01(float t) { return t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f; }

__host__ __device__ __forceinline__ float seg_d2(float px, float py, float pz, const float* __restrict__ s, const float* __restrict__ e) {
  const float dx = e[0] - s[0], dy = e[1] - s[1], dz = e[2] - s[2];
  const float wx = px - s[0], wy = py - s[1], wz = pz - s[2];
  const float dd = dot3(dx, dy, dz, dx, dy, dz);
  const float t = dd > 0.0f ? clamp01(dot3(wx, wy, wz, dx, dy, dz) / dd) : 0.0f;
  const float qx = wx - t * dx, qy = wy - t * dy, qz = wz - t * dz;
  return dot3(qx, qy, qz, qx, qy, qz);
}

// the definition's pair_d2 of face i
__host__ __device__ __forceinline__ float pair_d2(float px, float py, float pz, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                         int64_t i) {
  const int32_t ia = faces[i * 3], ib = faces[i * 3 + 1], ic = faces[i * 3 + 2];
  float a[3], b[3], c[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = vertices[(int64_t)ia * 3 + k];
    b[k] = vertices[(int64_t)ib * 3 + k];
    c[k] = vertices[(int64_t)ic * 3 + k];
  }
  const float e0 = ib < ia ? seg_d2(px, py, pz, b, a) : seg_d2(px, py, pz, a, b);
  const float e1 = ic < ib ? seg_d2(px, py, pz, c, b) : seg_d2(px, py, pz, b, c);
  const float e2 = ia < ic ? seg_d2(px, py, pz, a, c) : seg_d2(px, py, pz, c, a);
  float m = fminf(fminf(e0, e1), e2);
  const float abx = b[0] - a[0], aby = b[1] - a[1], abz = b[2] - a[2];
  const float acx = c[0] - a[0], acy = c[1] - a[1], acz = c[2] - a[2];
  const float wx = px - a[0], wy = py - a[1], wz = pz - a[2];
  const float abab = dot3(abx, aby, abz, abx, aby, abz), acac = dot3(acx, acy, acz, acx, acy, acz), abac = dot3(abx, aby, abz, acx, acy, acz);
  const float det = abab * acac - abac * abac;
  if (det > 0.0f) {
    const float d1 = dot3(wx, wy, wz, abx, aby, abz), d2 = dot3(wx, wy, wz, acx, acy, acz);
    const float s = clamp01((d1 * acac - d2 * abac) / det);
    const float r = 1.0f - s;
    float t = (d2 * abab - d1 * abac) / det;
    t = t > 0.0f ? (t < r ? t : r) : 0.0f;
    const float qx = (wx - s * abx) - t * acx, qy = (wy - s * aby) - t * acy, qz = (wz - s * abz) - t * acz;
    const float v = dot3(qx, qy, qz, qx, qy, qz);
    if (v < m) m = v;
  }
  return m;
}

// the cell coordinate of x on one axis, clamped into 0 .. n - 1 in FLOAT (x may be far outside), then an integer
__host__ __device__ __forceinline__ int cell_of(float x, float o, float inv_h, int n, float slack) {
  const float v = floorf((x - o) * inv_h + slack);
  return (int)fminf(fmaxf(v, 0.0f), (float)(n - 1));
}

__host__ __device__ __forceinline__ void face_cells(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t i, const Grid& g,
                                           FaceCells* t) {
  const int64_t ia = faces[i * 3], ib = faces[i * 3 + 1], ic = faces[i * 3 + 2];
  const float ax = vertices[ia * 3], ay = vertices[ia * 3 + 1], az = vertices[ia * 3 + 2];
  const float bx = vertices[ib * 3], by = vertices[ib * 3 + 1], bz = vertices[ib * 3 + 2];
  const float cx = vertices[ic * 3], cy = vertices[ic * 3 + 1], cz = vertices[ic * 3 + 2];
  t->x0 = cell_of(fminf(fminf(ax, bx), cx), g.ox, g.inv_h, g.nx, -BOX_SLACK);
  t->y0 = cell_of(fminf(fminf(ay, by), cy), g.oy, g.inv_h, g.ny, -BOX_SLACK);
  t->z0 = cell_of(fminf(fminf(az, bz), cz), g.oz, g.inv_h, g.nz, -BOX_SLACK);
  t->wx = cell_of(fmaxf(fmaxf(ax, bx), cx), g.ox, g.inv_h, g.nx, BOX_SLACK) - t->x0 + 1;
  t->wy = cell_of(fmaxf(fmaxf(ay, by), cy), g.oy, g.inv_h, g.ny, BOX_SLACK) - t->y0 + 1;
  t->wz = cell_of(fmaxf(fmaxf(az, bz), cz), g.oz, g.inv_h, g.nz, BOX_SLACK) - t->z0 + 1;
  const float abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
  t->ax = ax; t->ay = ay; t->az = az;
  t->nx = aby * acz - abz * acy;
  t->ny = abz * acx - abx * acz;
  t->nz = abx * acy - aby * acx;
  t->half = PLANE_HALF * g.h * ((fabsf(t->nx) + fabsf(t->ny)) + fabsf(t->nz));
  t->lablac = PLANE_ABS * ((fabsf(abx) + fabsf(aby)) + fabsf(abz)) * ((fabsf(acx) + fabsf(acy)) + fabsf(acz));
}

// does the face's plane, inflated by the rounding of everything involved, cross cell (x, y, z)?
__host__ __device__ __forceinline__ bool crossed(const FaceCells& t, const Grid& g, int x, int y, int z) {
  const float dx = (g.ox + ((float)x + 0.5f) * g.h) - t.ax;
  const float dy = (g.oy + ((float)y + 0.5f) * g.h) - t.ay;
  const float dz = (g.oz + ((float)z + 0.5f) * g.h) - t.az;
  const float dist = dot3(t.nx, t.ny, t.nz, dx, dy, dz);
  const float room = t.half + t.lablac * ((((fabsf(dx) + fabsf(dy)) + fabsf(dz)) + g.h) + g.vmax);
  return fabsf(dist) <= room;
}

template <bool FILL>
__device__ __forceinline__ void visit(const Grid& g, int x, int y, int z, uint32_t face, int32_t* __restrict__ counts,
                                      const int32_t* __restrict__ start, int32_t* __restrict__ entries) {
  const int64_t cell = ((int64_t)z * g.ny + y) * g.nx + x;
  if (!FILL) {
    atomicAdd(counts + cell, 1);
  } else {
    const int32_t slot = atomicAdd(counts + cell, 1), s = start[cell];
    if (slot >= 0 && slot < start[cell + 1] - s) entries[(int64_t)s + slot] = (int32_t)face;   // always true: fill repeats count
  }
}

template <bool FILL>
__global__ void __launch_bounds__(NT) faces_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t F, Grid g,
                                                   int32_t large_max, int32_t* __restrict__ counts, const int32_t* __restrict__ start,
                                                   int32_t* __restrict__ entries, uint32_t* __restrict__ counter,
                                                   uint32_t* __restrict__ queue) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  FaceCells t;
  const bool ok = i < F;
  if (ok) face_cells(vertices, faces, i, g, &t);
  const bool large = ok && (int64_t)t.wx * t.wy * t.wz > (int64_t)large_max;
  if (!FILL) {
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
        if (slot < (uint64_t)F) queue[slot] = (uint32_t)i;                                 // always true: a face enters once
      }
    }
  }
  if (!ok || large) return;
  for (int z = 0; z < t.wz; ++z)
    for (int y = 0; y < t.wy; ++y)
      for (int x = 0; x < t.wx; ++x)
        if (crossed(t, g, t.x0 + x, t.y0 + y, t.z0 + z)) visit<FILL>(g, t.x0 + x, t.y0 + y, t.z0 + z, (uint32_t)i, counts, start, entries);
}

template <bool FILL>
__global__ void __launch_bounds__(NT) large_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t F, Grid g,
                                                   int32_t* __restrict__ counts, const int32_t* __restrict__ start,
                                                   int32_t* __restrict__ entries, const uint32_t* __restrict__ counter,
                                                   const uint32_t* __restrict__ queue) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wave = (blockIdx.x * NT + threadIdx.x) / WAVE;
  const uint32_t waves = gridDim.x * (NT / WAVE);
  uint32_t count = *counter;
  if ((int64_t)count > F) count = (uint32_t)F;
  for (uint32_t q = wave; q < count; q += waves) {
    const int64_t i = queue[q];
    if (i >= F) continue;
    FaceCells t;
    face_cells(vertices, faces, i, g, &t);
    const int64_t n = (int64_t)t.wx * t.wy * t.wz, wxy = (int64_t)t.wx * t.wy;             // <= the grid's cells < 2^31
    for (int64_t k = lane; k < n; k += WAVE) {
      const int z = (int)(k / wxy), y = (int)((k % wxy) / t.wx), x = (int)(k % t.wx);
      if (crossed(t, g, t.x0 + x, t.y0 + y, t.z0 + z)) visit<FILL>(g, t.x0 + x, t.y0 + y, t.z0 + z, (uint32_t)i, counts, start, entries);
    }
  }
}

__global__ void __launch_bounds__(NT) blocks_kernel(const int32_t* __restrict__ start, Grid g, uint8_t* __restrict__ occupied) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int64_t nb = (int64_t)g.bx * g.by * g.bz;
  if (i >= nb) return;
  const int X = (int)(i % g.bx) * BLOCK, Y = (int)((i / g.bx) % g.by) * BLOCK, Z = (int)(i / ((int64_t)g.bx * g.by)) * BLOCK;
  const int x1 = min(X + BLOCK, g.nx), y1 = min(Y + BLOCK, g.ny), z1 = min(Z + BLOCK, g.nz);
  bool any = false;
  for (int z = Z; z < z1; ++z)
    for (int y = Y; y < y1; ++y) {
      const int64_t row = ((int64_t)z * g.ny + y) * g.nx;                                  // the cells of a row are contiguous
      any = any || start[row + x1] > start[row + X];
    }
  occupied[i] = any ? 1 : 0;
}

// the flags of the super blocks follow those of the blocks in `occupied`
__global__ void __launch_bounds__(NT) supers_kernel(Grid g, uint8_t* __restrict__ occupied) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int64_t nb = (int64_t)g.bx * g.by * g.bz, ns = (int64_t)g.sx * g.sy * g.sz;
  if (i >= ns) return;
  const int X = (int)(i % g.sx) * SUPER, Y = (int)((i / g.sx) % g.sy) * SUPER, Z = (int)(i / ((int64_t)g.sx * g.sy)) * SUPER;
  const int x1 = min(X + SUPER, g.bx), y1 = min(Y + SUPER, g.by), z1 = min(Z + SUPER, g.bz);
  bool any = false;
  for (int z = Z; z < z1; ++z)
    for (int y = Y; y < y1; ++y)
      for (int x = X; x < x1; ++x) any = any || occupied[((int64_t)z * g.by + y) * g.bx + x] != 0;
  occupied[nb + i] = any ? 1 : 0;
}

// lb2 of step 3 from one axis' index offset k >= 0
__host__ __device__ __forceinline__ float axis_gap(int k, float h) { return fmaxf((float)(k - 1) - BOX_SLACK, 0.0f) * h; }

struct Best {
  float d2, thr2, eta;
  uint32_t face;
};

__host__ __device__ __forceinline__ void offer(Best* b, float d, uint32_t f) {
  if (d < b->d2 || (d == b->d2 && f < b->face)) {
    b->d2 = d;
    b->face = f;
    const float thr = (sqrtf(d) + b->eta) * UP;
    b->thr2 = (thr * thr) * UP;
  }
}

// BOUNDED: only candidates with pair_d2 <= max_d2 are offered (step 5); max_d2 is not read otherwise
template <bool BOUNDED>
__host__ __device__ __forceinline__ void walk_block(const Grid& g, int BX, int BY, int BZ, int c0x, int c0y, int c0z, float px, float py, float pz,
                                           const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                           const int32_t* __restrict__ start, const int32_t* __restrict__ entries,
                                           const uint8_t* __restrict__ occupied, float max_d2, Best* best) {
  if (!occupied[((int64_t)BZ * g.by + BY) * g.bx + BX]) return;
  const int X = BX * BLOCK, Y = BY * BLOCK, Z = BZ * BLOCK;
  {
    const float gx = axis_gap(imax(imax(X - c0x, c0x - (X + BLOCK - 1)), 0), g.h);
    const float gy = axis_gap(imax(imax(Y - c0y, c0y - (Y + BLOCK - 1)), 0), g.h);
    const float gz = axis_gap(imax(imax(Z - c0z, c0z - (Z + BLOCK - 1)), 0), g.h);
    if ((gx * gx + gy * gy) + gz * gz > best->thr2) return;
  }
  const int x1 = imin(X + BLOCK, g.nx), y1 = imin(Y + BLOCK, g.ny), z1 = imin(Z + BLOCK, g.nz);
  for (int z = Z; z < z1; ++z) {
    const float gz = axis_gap(iabs(z - c0z), g.h);
    for (int y = Y; y < y1; ++y) {
      const float gy = axis_gap(iabs(y - c0y), g.h);
      const int64_t row = ((int64_t)z * g.ny + y) * g.nx;
      for (int x = X; x < x1; ++x) {
        const int32_t s = start[row + x], e = start[row + x + 1];
        if (e <= s) continue;
        const float gx = axis_gap(iabs(x - c0x), g.h);
        if ((gx * gx + gy * gy) + gz * gz > best->thr2) continue;
        for (int32_t j = s; j < e; ++j) {
          const uint32_t f = (uint32_t)entries[j];
          if (f == best->face) continue;                                                   // the same face from another cell
          const float d = pair_d2(px, py, pz, vertices, faces, (int64_t)f);
          if (!BOUNDED || d <= max_d2) offer(best, d, f);                                  // a NaN is not offered
        }
      }
    }
  }
}

// the blocks of one occupied super block that the bound lets through
template <bool BOUNDED>
__host__ __device__ __forceinline__ void walk_super(const Grid& g, int SX, int SY, int SZ, int c0x, int c0y, int c0z, float px, float py, float pz,
                                                    const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                    const int32_t* __restrict__ start, const int32_t* __restrict__ entries,
                                                    const uint8_t* __restrict__ occupied, float max_d2, Best* best) {
  const int64_t nb = (int64_t)g.bx * g.by * g.bz;
  if (!occupied[nb + ((int64_t)SZ * g.sy + SY) * g.sx + SX]) return;
  constexpr int EDGE = BLOCK * SUPER;                                                      // cells
  const int X = SX * EDGE, Y = SY * EDGE, Z = SZ * EDGE;
  const float gx = axis_gap(imax(imax(X - c0x, c0x - (X + EDGE - 1)), 0), g.h);
  const float gy = axis_gap(imax(imax(Y - c0y, c0y - (Y + EDGE - 1)), 0), g.h);
  const float gz = axis_gap(imax(imax(Z - c0z, c0z - (Z + EDGE - 1)), 0), g.h);
  if ((gx * gx + gy * gy) + gz * gz > best->thr2) return;
  const int x1 = imin((SX + 1) * SUPER, g.bx), y1 = imin((SY + 1) * SUPER, g.by), z1 = imin((SZ + 1) * SUPER, g.bz);
  for (int BZ = SZ * SUPER; BZ < z1; ++BZ)
    for (int BY = SY * SUPER; BY < y1; ++BY)
      for (int BX = SX * SUPER; BX < x1; ++BX)
        walk_block<BOUNDED>(g, BX, BY, BZ, c0x, c0y, c0z, px, py, pz, vertices, faces, start, entries, occupied, max_d2, best);
}

// the whole query of one point -> (d2, face); (inf, all ones) for a point with a non-finite coordinate and, BOUNDED, for one
// without a face within max_d2.  max_root = sqrtf(max_d2), taken once by the host: both are the same for every point.
template <bool BOUNDED>
__host__ __device__ __forceinline__ Best query_point(float px, float py, float pz, const Grid& g, const float* __restrict__ vertices,
                                                     const int32_t* __restrict__ faces, const int32_t* __restrict__ start,
                                                     const int32_t* __restrict__ entries, const uint8_t* __restrict__ occupied,
                                                     float max_d2, float max_root) {
  Best best;
  best.d2 = INFINITY;
  best.thr2 = INFINITY;
  best.eta = 0.0f;
  best.face = 0xffffffffu;
  if (!(fabsf(px) < INFINITY && fabsf(py) < INFINITY && fabsf(pz) < INFINITY)) return best;  // NaN too
  best.eta = ETA * (fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz)) + 4.0f * g.vmax);
  if (BOUNDED) {                                                                           // step 5: the point's own cap
    const float cap_thr = (max_root + best.eta) * UP;
    best.thr2 = (cap_thr * cap_thr) * UP;
  }
  const int c0x = cell_of(px, g.ox, g.inv_h, g.nx, 0.0f), c0y = cell_of(py, g.oy, g.inv_h, g.ny, 0.0f),
            c0z = cell_of(pz, g.oz, g.inv_h, g.nz, 0.0f);
  constexpr int EDGE = BLOCK * SUPER;
  const int Cx = c0x / EDGE, Cy = c0y / EDGE, Cz = c0z / EDGE;
  const int rings = imax(imax(imax(Cx, g.sx - 1 - Cx), imax(Cy, g.sy - 1 - Cy)), imax(Cz, g.sz - 1 - Cz));
  for (int K = 0; K <= rings; ++K) {
    if (K >= 2) {
      // a super block of ring K starts at least EDGE K - (EDGE - 1) cells from the point's cell on some axis
      const float gap = axis_gap(EDGE * K - (EDGE - 1), g.h);
      if (gap * gap > best.thr2) break;
    }
    const int z0 = imax(Cz - K, 0), z1 = imin(Cz + K, g.sz - 1), y0 = imax(Cy - K, 0), y1 = imin(Cy + K, g.sy - 1);
    const int x0 = imax(Cx - K, 0), x1 = imin(Cx + K, g.sx - 1);
    for (int SZ = z0; SZ <= z1; ++SZ)
      for (int SY = y0; SY <= y1; ++SY) {
        if (iabs(SZ - Cz) == K || iabs(SY - Cy) == K) {
          for (int SX = x0; SX <= x1; ++SX)
            walk_super<BOUNDED>(g, SX, SY, SZ, c0x, c0y, c0z, px, py, pz, vertices, faces, start, entries, occupied, max_d2, &best);
        } else {                                                                           // K > 0: only the two ends of the row
          if (Cx - K >= 0) walk_super<BOUNDED>(g, Cx - K, SY, SZ, c0x, c0y, c0z, px, py, pz, vertices, faces, start, entries, occupied, max_d2, &best);
          if (Cx + K < g.sx) walk_super<BOUNDED>(g, Cx + K, SY, SZ, c0x, c0y, c0z, px, py, pz, vertices, faces, start, entries, occupied, max_d2, &best);
        }
      }
  }
  return best;
}

__global__ void __launch_bounds__(NT) query_kernel(const float* __restrict__ points, int64_t N, const int64_t* __restrict__ order,
                                                   const float* __restrict__ vertices, const int32_t* __restrict__ faces, Grid g,
                                                   const int32_t* __restrict__ start, const int32_t* __restrict__ entries,
                                                   const uint8_t* __restrict__ occupied, float* __restrict__ out_d2,
                                                   int32_t* __restrict__ out_face) {
  const int64_t k = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (k >= N) return;
  const int64_t i = order ? order[k] : k;
  if (i < 0 || i >= N) return;                                                             // a permutation: never
  const Best best = query_point<false>(points[i * 3], points[i * 3 + 1], points[i * 3 + 2], g, vertices, faces, start, entries, occupied,
                                       0.0f, 0.0f);
  out_d2[i] = best.d2;
  out_face[i] = (int32_t)best.face;                                                        // all ones -> -1
}

// the bounded form: max_d2 and max_root are kernel arguments, the same for the whole launch; the cap they give is per point
__global__ void __launch_bounds__(NT) query_bounded_kernel(const float* __restrict__ points, int64_t N, const int64_t* __restrict__ order,
                                                           const float* __restrict__ vertices, const int32_t* __restrict__ faces, Grid g,
                                                           const int32_t* __restrict__ start, const int32_t* __restrict__ entries,
                                                           const uint8_t* __restrict__ occupied, float max_d2, float max_root,
                                                           float* __restrict__ out_d2, int32_t* __restrict__ out_face) {
  const int64_t k = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (k >= N) return;
  const int64_t i = order ? order[k] : k;
  if (i < 0 || i >= N) return;                                                             // a permutation: never
  const Best best = query_point<true>(points[i * 3], points[i * 3 + 1], points[i * 3 + 2], g, vertices, faces, start, entries, occupied,
                                      max_d2, max_root);
  out_d2[i] = best.d2;
  out_face[i] = (int32_t)best.face;                                                        // all ones -> -1: nothing within the bound
}

__global__ void __launch_bounds__(NT) keys_kernel(const float* __restrict__ points, int64_t N, Grid g, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= N) return;
  const float px = points[i * 3], py = points[i * 3 + 1], pz = points[i * 3 + 2];
  int64_t key = 0;
  if (fabsf(px) < INFINITY && fabsf(py) < INFINITY && fabsf(pz) < INFINITY) {
    // block-major, so that the points of one block are neighbours in the sorted order
    const int x = cell_of(px, g.ox, g.inv_h, g.nx, 0.0f), y = cell_of(py, g.oy, g.inv_h, g.ny, 0.0f), z = cell_of(pz, g.oz, g.inv_h, g.nz, 0.0f);
    const int64_t blk = ((int64_t)(z / BLOCK) * g.by + y / BLOCK) * g.bx + x / BLOCK;
    key = blk * (BLOCK * BLOCK * BLOCK) + ((z % BLOCK) * BLOCK + y % BLOCK) * BLOCK + x % BLOCK;
  }
  keys[i] = key;
}

__global__ void __launch_bounds__(NT) normals_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t F,
                                                     const int32_t* __restrict__ face, int64_t N, float* __restrict__ normals) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= N) return;
  const int64_t f = face[i];
  float a[3], n[3] = {0.0f, 0.0f, 0.0f};
  if (f >= 0 && f < F) rtgs_face_unit_normal(vertices, faces, f, a, n);                    // mesh_face_normal.h
  normals[i * 3] = n[0]; normals[i * 3 + 1] = n[1]; normals[i * 3 + 2] = n[2];
}

inline bool make_grid(const float* origin_host, float cell, const int32_t* dims_host, float vmax, Grid* g) {
  if (!origin_host || !dims_host || !(cell > 0.0f) || !(cell < INFINITY) || !(vmax >= 0.0f) || !(vmax <= 1048576.0f)) return false;
  for (int k = 0; k < 3; ++k)
    if (!(fabsf(origin_host[k]) < INFINITY) || dims_host[k] < 1 || dims_host[k] > MAX_DIM) return false;
  if ((int64_t)dims_host[0] * dims_host[1] * dims_host[2] > 0x7fffffffLL) return false;
  g->ox = origin_host[0]; g->oy = origin_host[1]; g->oz = origin_host[2];
  g->h = cell;
  g->inv_h = 1.0f / cell;
  if (!(g->inv_h > 0.0f) || !(g->inv_h < INFINITY)) return false;
  g->nx = dims_host[0]; g->ny = dims_host[1]; g->nz = dims_host[2];
  g->bx = (g->nx + BLOCK - 1) / BLOCK; g->by = (g->ny + BLOCK - 1) / BLOCK; g->bz = (g->nz + BLOCK - 1) / BLOCK;
  g->sx = (g->bx + SUPER - 1) / SUPER; g->sy = (g->by + SUPER - 1) / SUPER; g->sz = (g->bz + SUPER - 1) / SUPER;
  g->vmax = vmax;
  return true;
}

template <bool FILL>
int register_faces(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const float* origin_host, float cell,
                   const int32_t* dims_host, float vmax, int32_t large_max, int32_t* counts, const int32_t* start, int32_t* entries,
                   void* queue_scratch, void* stream) {
  Grid g;
  if (V <= 0 || F <= 0 || F >= 0x80000000LL || !vertices || !faces || large_max < 0 || !counts || !queue_scratch) return -1;
  if (FILL && (!start || !entries)) return -1;
  if (!make_grid(origin_host, cell, dims_host, vmax, &g)) return -1;
  unsigned face_blocks;
  if (!grid_for(F, &face_blocks)) return -1;
  uint32_t* counter = (uint32_t*)queue_scratch;
  uint32_t* queue = (uint32_t*)((char*)queue_scratch + 16);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(faces_kernel<FILL>, dim3(face_blocks), dim3(NT), 0, s, vertices, faces, F, g, large_max, counts, start, entries, counter,
                     queue);
  const int64_t one_wave_each = (F + NT / WAVE - 1) / (NT / WAVE);
  const unsigned large_blocks = (unsigned)(one_wave_each < LARGE_BLOCKS ? one_wave_each : LARGE_BLOCKS);
  hipLaunchKernelGGL(large_kernel<FILL>, dim3(large_blocks), dim3(NT), 0, s, vertices, faces, F, g, counts, start, entries, counter, queue);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace rtgs_mesh_distance_k

extern "C" {

using namespace rtgs_mesh_distance_k;

size_t rtgs_mesh_distance_queue_bytes(int64_t F) {
  if (F < 0 || F >= 0x80000000LL) return 0;
  return 16 + (size_t)F * sizeof(uint32_t);
}

int rtgs_mesh_distance_count(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const float* origin_host, float cell,
                             const int32_t* dims_host, float vmax, int32_t large_max, int32_t* counts, void* queue_scratch, void* stream) {
  return register_faces<false>(vertices, V, faces, F, origin_host, cell, dims_host, vmax, large_max, counts, nullptr, nullptr, queue_scratch,
                               stream);
}

int rtgs_mesh_distance_fill(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const float* origin_host, float cell,
                            const int32_t* dims_host, float vmax, int32_t large_max, const int32_t* start, int32_t* cursor, int32_t* entries,
                            void* queue_scratch, void* stream) {
  return register_faces<true>(vertices, V, faces, F, origin_host, cell, dims_host, vmax, large_max, cursor, start, entries, queue_scratch,
                              stream);
}

int rtgs_mesh_distance_blocks(const int32_t* start, const float* origin_host, float cell, const int32_t* dims_host, uint8_t* occupied,
                              void* stream) {
  Grid g;
  if (!start || !occupied || !make_grid(origin_host, cell, dims_host, 0.0f, &g)) return -1;
  unsigned blocks;
  if (!grid_for((int64_t)g.bx * g.by * g.bz, &blocks)) return -1;
  hipLaunchKernelGGL(blocks_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, start, g, occupied);
  unsigned supers;
  if (!grid_for((int64_t)g.sx * g.sy * g.sz, &supers)) return -1;
  hipLaunchKernelGGL(supers_kernel, dim3(supers), dim3(NT), 0, (hipStream_t)stream, g, occupied);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_mesh_distance_query(const float* points, int64_t N, const int64_t* order, const float* vertices, int64_t V, const int32_t* faces,
                             int64_t F, const float* origin_host, float cell, const int32_t* dims_host, float vmax, const int32_t* start,
                             const int32_t* entries, const uint8_t* occupied, float* d2, int32_t* face, void* stream) {
  Grid g;
  if (N < 0 || V <= 0 || F <= 0 || F >= 0x80000000LL || !vertices || !faces || !start || !entries || !occupied) return -1;
  if (!make_grid(origin_host, cell, dims_host, vmax, &g)) return -1;
  if (N == 0) return 0;
  if (!points || !d2 || !face) return -1;
  unsigned blocks;
  if (!grid_for(N, &blocks)) return -1;
  hipLaunchKernelGGL(query_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, points, N, order, vertices, faces, g, start, entries,
                     occupied, d2, face);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_mesh_distance_query_bounded(const float* points, int64_t N, const int64_t* order, const float* vertices, int64_t V,
                                     const int32_t* faces, int64_t F, const float* origin_host, float cell, const int32_t* dims_host, float vmax,
                                     const int32_t* start, const int32_t* entries, const uint8_t* occupied, float max_d2, float* d2,
                                     int32_t* face, void* stream) {
  Grid g;
  if (N < 0 || V <= 0 || F <= 0 || F >= 0x80000000LL || !vertices || !faces || !start || !entries || !occupied) return -1;
  if (!(max_d2 >= 0.0f)) return -1;                                                        // NaN too
  if (!make_grid(origin_host, cell, dims_host, vmax, &g)) return -1;
  if (N == 0) return 0;
  if (!points || !d2 || !face) return -1;
  unsigned blocks;
  if (!grid_for(N, &blocks)) return -1;
  hipLaunchKernelGGL(query_bounded_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, points, N, order, vertices, faces, g, start,
                     entries, occupied, max_d2, sqrtf(max_d2), d2, face);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_mesh_distance_keys(const float* points, int64_t N, const float* origin_host, float cell, const int32_t* dims_host, int64_t* keys,
                            void* stream) {
  Grid g;
  if (N < 0 || !make_grid(origin_host, cell, dims_host, 0.0f, &g)) return -1;
  if (N == 0) return 0;
  if (!points || !keys) return -1;
  unsigned blocks;
  if (!grid_for(N, &blocks)) return -1;
  hipLaunchKernelGGL(keys_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, points, N, g, keys);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_mesh_distance_normals(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int32_t* face, int64_t N,
                               float* normals, void* stream) {
  if (N < 0 || V <= 0 || F <= 0 || !vertices || !faces) return -1;
  if (N == 0) return 0;
  if (!face || !normals) return -1;
  unsigned blocks;
  if (!grid_for(N, &blocks)) return -1;
  hipLaunchKernelGGL(normals_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, vertices, faces, F, face, N, normals);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
