// gfx950 kernels + C ABI of the mesher (include/rtgs_slam.h, "meshing"): TSDF fusion of one depth / colour frame into a dense
// grid, and marching tetrahedra on the Freudenthal split of its cells.  The reference has no mesher; tests/tsdf_reference.py
// restates both in numpy and is the definition.
//
// Volume: corner lo, dims (nx, ny, nz), edge `voxel`, x fastest; planes tsdf, weight [nz][ny][nx] and rgb [3][nz][ny][nx], all
// float32.  Voxel (ix, iy, iz) has linear index (iz ny + iy) nx + ix and centre lo + ((float)i + 0.5f) voxel per axis.
//
// Integration float chain (float32, one correctly rounded operation per step; built with -ffp-contract=off, Makefile
// EXTRA_tsdf): integrate_voxel below, steps 1-12 of the header comment.
//
// Two forms of the integration launch, selected by rtgs_tsdf_set_dense (include/rtgs_debug.h), identical planes:
// Both first run pack_frame_kernel: colour and depth interleaved as float4, and the frame's largest valid depth.
//   dense  one thread per voxel over the whole grid; every thread projects its voxel, only the ones that update touch memory.
//   block  (default) one wave per BX x BY x BZ = 64 x 8 x 1 block, a lane per x and 8 voxels a lane, so that every access of
//          a wave to a plane is 256 contiguous bytes, as in the dense form.  The wave's lanes transform the block's 8
//          corner centres and six ballots decide whether the whole block can be skipped: every corner behind the camera,
//          every corner farther than the frame's largest depth + trunc, or every corner outside one of the four side planes
//          of the frustum.  Camera-space coordinates and the side-plane forms L = f x_c + (c + 0.5 [- size]) z_c are affine
//          in the voxel centre, so their extremes over the block sit at its corners; the margins (m_z, m_x, m_y: about 170
//          ulp of the largest magnitude the chain can reach in this volume) cover the rounding of the per-voxel chain, so a
//          skipped block holds no voxel the dense form would have updated.  No LDS, no barrier.
//
// Extraction: a cell (lower-corner voxel v, all 8 corners with weight >= min_weight) is split into the 6 tetrahedra around its
// main diagonal: for every permutation (a, b, c) of the axes, corners 0, e_a, e_a + e_b, 7 (bit 0 = +x, bit 1 = +y, bit 2 =
// +z).  Every tetrahedron edge runs from a corner to one that contains its bits, so it belongs to one of the 7 classes (the
// direction bits 1..7) of its lower endpoint's voxel: key = (lower endpoint's linear index) 7 + (direction - 1).  The 16-case
// table is generated at compile time (make_table); orientation is fixed there with the crossings at the edge midpoints in
// integer arithmetic.  A crossing is interpolated from the lower linear index a to the higher b:
//   w = t_a / (t_a - t_b),  p = p_a + (p_b - p_a) w,  colour likewise.
//
// The sparse brick volume (rtgs_tsdf_sparse_*; tests/tsdf_sparse_reference.py is its definition): the same virtual grid with
// planes only for the 8 x 8 x 8 bricks near an observed surface - a table of one int32 per brick (slot or -1), a pool
// [slot][tsdf, weight, r, g, b][z][y][x] of 10 240 B a brick, the slots' brick coordinates.  project_voxel / observe / fuse,
// the brick test (box_outside) and the case table are the dense form's, so an allocated voxel follows the same float chain.
//   mark       one wave per brick of the virtual grid; the six-ballot test, then the brick's voxels are projected and tested in
//              band (updated by the dense rule, s < 1); an in-band voxel flags its brick and the face / edge / corner
//              neighbours it touches, where they have no slot yet (plain stores of 1)
//   allocate   the caller scans the flags in brick-linear order and reads their sum; new bricks get the slots after the old
//              ones in that order, their coordinates are recorded and their planes made fresh
//   integrate  one wave per allocated brick, a lane per (x, y), the 8 z layers in two batched passes: 256 contiguous bytes per
//              access of a wave to a plane, no LDS, no barrier
//   count/emit one wave per allocated brick; lanes 0..7 look up the slots of the brick and its 7 upper neighbours once; 64-bit
//              linear indices and keys; triangles leave in slot order with their cell's linear index for the caller's sort
#include "../../include/rtgs_slam.h"
#include "../../include/rtgs_debug.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace rtgs_tsdf {

constexpr int NT = 256;
constexpr int BX = 64, BY = 8, BZ = 1;

struct Grid {
  int nx, ny, nz;
  float lox, loy, loz, voxel;
};

struct Frame {
  float r[9], t[3];            // world-to-camera, rows
  float fx, fy, cx, cy;
  int H, W;
  float trunc, max_weight;
  float mz, mx, my;            // margins of the block test
};

__device__ __forceinline__ void to_camera(const Frame& f, float x, float y, float z, float& xc, float& yc, float& zc) {
  xc = ((f.r[0] * x + f.r[1] * y) + f.r[2] * z) + f.t[0];
  yc = ((f.r[3] * x + f.r[4] * y) + f.r[5] * z) + f.t[1];
  zc = ((f.r[6] * x + f.r[7] * y) + f.r[8] * z) + f.t[2];
}

// steps 1-6: the voxel's pixel (row-major index) and camera depth; false when it is behind the camera or outside the image
__device__ __forceinline__ bool project_voxel(const Grid& g, const Frame& f, int ix, int iy, int iz, int& pix, float& zc) {
  const float x = g.lox + ((float)ix + 0.5f) * g.voxel;
  const float y = g.loy + ((float)iy + 0.5f) * g.voxel;
  const float z = g.loz + ((float)iz + 0.5f) * g.voxel;
  float xc, yc;
  to_camera(f, x, y, z, xc, yc, zc);
  if (!(zc > 0.0f)) return false;
  const float u = f.fx * xc / zc + f.cx;
  const float v = f.fy * yc / zc + f.cy;
  const float pu = floorf(u + 0.5f), pv = floorf(v + 0.5f);
  if (!(pu >= 0.0f && pu < (float)f.W && pv >= 0.0f && pv < (float)f.H)) return false;     // also drops NaN / inf
  pix = (int)pv * f.W + (int)pu;
  return true;
}

// steps 7-9: false for a hole or a voxel more than trunc behind the surface
__device__ __forceinline__ bool observe(const Frame& f, float d, float zc, float& s) {
  if (!(d > 0.0f)) return false;
  const float sdf = d - zc;
  if (sdf < -f.trunc) return false;
  s = fminf(1.0f, sdf / f.trunc);
  return true;
}

// steps 10-12 on loaded values
__device__ __forceinline__ float fuse(float old, float w, float obs, float w1) { return (old * w + obs) / w1; }

__device__ __forceinline__ void integrate_voxel(const Grid& g, const Frame& f, int ix, int iy, int iz, int64_t plane,
                                                const float4* __restrict__ frame, float* __restrict__ tsdf,
                                                float* __restrict__ weight, float* __restrict__ rgb) {
  int pix;
  float zc, s;
  if (!project_voxel(g, f, ix, iy, iz, pix, zc)) return;
  const float4 q = frame[pix];                                 // r, g, b, depth
  if (!observe(f, q.w, zc, s)) return;
  const int64_t i = ((int64_t)iz * g.ny + iy) * g.nx + ix;
  const float w = weight[i];
  const float w1 = w + 1.0f;
  tsdf[i] = fuse(tsdf[i], w, s, w1);
  rgb[i] = fuse(rgb[i], w, q.x, w1);
  rgb[plane + i] = fuse(rgb[plane + i], w, q.y, w1);
  rgb[2 * plane + i] = fuse(rgb[2 * plane + i], w, q.z, w1);
  weight[i] = fminf(w1, f.max_weight);
}

// One pass over the frame before the voxels: colour and depth interleaved as float4 (r, g, b, depth), so that a voxel's four
// gathers - the dominant memory transactions of a frame seen from inside the volume, where neighbouring voxels project
// pixels apart - become one 16-B load; and the frame's largest valid depth, as the bits of a positive float (they order as
// unsigned integers), one atomic per workgroup.
constexpr int PACK_GROUPS = 256;

__global__ void __launch_bounds__(NT) pack_frame_kernel(const float* __restrict__ depth, const float* __restrict__ color, int64_t n,
                                                        float4* __restrict__ frame, uint32_t* __restrict__ out) {
  __shared__ uint32_t part[NT / 64];
  uint32_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
    const float d = depth[i];
    frame[i] = make_float4(color[i], color[n + i], color[2 * n + i], d);
    if (d > 0.0f && d <= 3.0e38f) m = max(m, __float_as_uint(d));
    else if (d > 3.0e38f) m = 0x7f800000u;
  }
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < NT / 64; ++k) m = max(m, part[k]);
    if (m != 0) atomicMax(out, m);
  }
}

__global__ void __launch_bounds__(NT) integrate_dense_kernel(Grid g, Frame f, const float4* __restrict__ frame,
                                                             float* __restrict__ tsdf, float* __restrict__ weight,
                                                             float* __restrict__ rgb) {
  const int64_t plane = (int64_t)g.nx * g.ny * g.nz;
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= plane) return;
  const int ix = (int)(i % g.nx);
  const int64_t r = i / g.nx;
  integrate_voxel(g, f, ix, (int)(r % g.ny), (int)(r / g.ny), plane, frame, tsdf, weight, rgb);
}

// The six-ballot test of the box of voxels [x0, x1] x [y0, y1] x [z0, z1] (inclusive), by a whole wave: lanes 0..7 (every
// lane, by lane & 7) transform the box's corner centres; true when every corner is behind the camera, farther than the
// frame's largest depth + trunc, or outside one of the four side planes of the frustum, so that no voxel of the box updates.
__device__ __forceinline__ bool box_outside(const Grid& g, const Frame& f, int lane, int x0, int y0, int z0, int x1, int y1, int z1,
                                            const uint32_t* __restrict__ dmax_bits) {
  const int c = lane & 7;
  const float x = g.lox + ((float)((c & 1) ? x1 : x0) + 0.5f) * g.voxel;
  const float y = g.loy + ((float)((c & 2) ? y1 : y0) + 0.5f) * g.voxel;
  const float z = g.loz + ((float)((c & 4) ? z1 : z0) + 0.5f) * g.voxel;
  float xc, yc, zc;
  to_camera(f, x, y, z, xc, yc, zc);
  const float dmax = __uint_as_float(*dmax_bits);
  const float lx = f.fx * xc, ly = f.fy * yc;
  const bool behind = zc < -f.mz;
  const bool beyond = zc - f.mz > (dmax + f.trunc) + f.mz;
  const bool left = lx + (f.cx + 0.5f) * zc < -f.mx;
  const bool right = lx + (f.cx + 0.5f - (float)f.W) * zc > f.mx;
  const bool top = ly + (f.cy + 0.5f) * zc < -f.my;
  const bool bottom = ly + (f.cy + 0.5f - (float)f.H) * zc > f.my;
  const auto all8 = [](bool p) { return (__ballot(p) & 0xffull) == 0xffull; };
  return !(dmax > 0.0f) || all8(behind) || all8(beyond) || all8(left) || all8(right) || all8(top) || all8(bottom);
}

// One WAVE per block, no LDS and no barrier: lanes 0..7 (every lane, by lane & 7) transform the block's corner centres, six
// ballots decide; a wave that stays walks its block with a lane per x (256 contiguous bytes of a plane per access) in passes
// of PV rows, each pass as batches - project and gather the pixel of all PV, then load the planes of the ones that update,
// then fuse and store - so that the loads of a pass are in flight together.
constexpr int WAVES = NT / 64;
constexpr int PV = 4;
static_assert(BX == 64 && (BY * BZ) % PV == 0, "a lane per x, BY BZ voxels a lane in passes of PV");

__global__ void __launch_bounds__(NT) integrate_block_kernel(Grid g, Frame f, int nbx, int nby, int64_t nblocks,
                                                             const float4* __restrict__ frame,
                                                             const uint32_t* __restrict__ dmax_bits, float* __restrict__ tsdf,
                                                             float* __restrict__ weight, float* __restrict__ rgb) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (b >= nblocks) return;                                   // wave-uniform
  const int x0 = (int)(b % nbx) * BX, y0 = (int)((b / nbx) % nby) * BY, z0 = (int)(b / ((int64_t)nbx * nby)) * BZ;
  if (box_outside(g, f, lane, x0, y0, z0, min(x0 + BX, g.nx) - 1, min(y0 + BY, g.ny) - 1, min(z0 + BZ, g.nz) - 1, dmax_bits)) return;
  const int64_t plane = (int64_t)g.nx * g.ny * g.nz;
  const int ix = x0 + lane;
#pragma unroll
  for (int pass = 0; pass < BY * BZ / PV; ++pass) {
    int pix[PV];
    int64_t idx[PV];
    float zc[PV], s[PV], w[PV], t[PV], c[PV][3];
    float4 q[PV];
    bool ok[PV];
#pragma unroll
    for (int v = 0; v < PV; ++v) {
      const int n = pass * PV + v;
      const int iy = y0 + n % BY, iz = z0 + n / BY;
      int p = 0;
      zc[v] = 0.0f;
      ok[v] = ix < g.nx && iy < g.ny && iz < g.nz && project_voxel(g, f, ix, iy, iz, p, zc[v]);
      pix[v] = ok[v] ? p : 0;
      idx[v] = ((int64_t)iz * g.ny + iy) * g.nx + ix;
      q[v] = frame[pix[v]];                                    // pixel 0 for a voxel that does not project: never used
    }
#pragma unroll
    for (int v = 0; v < PV; ++v) {
      s[v] = 0.0f;
      ok[v] = ok[v] && observe(f, q[v].w, zc[v], s[v]);
      if (ok[v]) {
        w[v] = weight[idx[v]];
        t[v] = tsdf[idx[v]];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[v][k] = rgb[k * plane + idx[v]];
      }
    }
#pragma unroll
    for (int v = 0; v < PV; ++v) {
      if (ok[v]) {
        const float w1 = w[v] + 1.0f;
        tsdf[idx[v]] = fuse(t[v], w[v], s[v], w1);
        const float o[3] = {q[v].x, q[v].y, q[v].z};
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[k * plane + idx[v]] = fuse(c[v][k], w[v], o[k], w1);
        weight[idx[v]] = fminf(w1, f.max_weight);
      }
    }
  }
}

// ---- marching tetrahedra ------------------------------------------------------------------------------------------------
struct Table {
  uint8_t ntri[6][16];
  uint8_t edge[6][16][6];      // per triangle vertex: (lower corner << 3) | upper corner
  uint8_t corner[6][4];
};

constexpr int cbit(int c, int axis) { return (c >> axis) & 1; }

constexpr Table make_table() {
  Table T{};
  const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int t = 0; t < 6; ++t) {
    int v[4] = {0, 1 << perms[t][0], (1 << perms[t][0]) | (1 << perms[t][1]), 7};
    for (int k = 0; k < 4; ++k) T.corner[t][k] = (uint8_t)v[k];
    for (int m = 0; m < 16; ++m) {
      int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
      for (int k = 0; k < 4; ++k) {
        if ((m >> k) & 1) in[ni++] = k; else out[no++] = k;
      }
      int tri[2][3][2] = {};   // [triangle][vertex][the two local vertices of the crossed edge]
      int nt = 0;
      if (ni == 1 || ni == 3) {
        const int p = ni == 1 ? in[0] : out[0];
        const int* o = ni == 1 ? out : in;
        for (int k = 0; k < 3; ++k) { tri[0][k][0] = p; tri[0][k][1] = o[k]; }
        nt = 1;
      } else if (ni == 2) {
        const int p = in[0], q = in[1], r = out[0], s = out[1];
        const int quad[4][2] = {{p, r}, {p, s}, {q, s}, {q, r}};
        const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
        for (int j = 0; j < 2; ++j)
          for (int k = 0; k < 3; ++k) { tri[j][k][0] = quad[pick[j][k]][0]; tri[j][k][1] = quad[pick[j][k]][1]; }
        nt = 2;
      }
      // direction from the inside corners to the outside ones, times ni no (integer)
      int dir[3] = {0, 0, 0};
      for (int a = 0; a < 3; ++a) {
        int si = 0, so = 0;
        for (int k = 0; k < ni; ++k) si += cbit(v[in[k]], a);
        for (int k = 0; k < no; ++k) so += cbit(v[out[k]], a);
        dir[a] = so * ni - si * no;
      }
      for (int j = 0; j < nt; ++j) {
        int P[3][3] = {};      // crossings at the edge midpoints, times 2
        for (int k = 0; k < 3; ++k)
          for (int a = 0; a < 3; ++a) P[k][a] = cbit(v[tri[j][k][0]], a) + cbit(v[tri[j][k][1]], a);
        const int e1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
        const int e2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
        const int n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const int dot = n[0] * dir[0] + n[1] * dir[1] + n[2] * dir[2];
        if (dot < 0) {
          for (int a = 0; a < 2; ++a) { const int sw = tri[j][1][a]; tri[j][1][a] = tri[j][2][a]; tri[j][2][a] = sw; }
        }
        for (int k = 0; k < 3; ++k) {
          const int c0 = v[tri[j][k][0]], c1 = v[tri[j][k][1]];
          const int lo = c0 < c1 ? c0 : c1, hi = c0 < c1 ? c1 : c0;
          T.edge[t][m][3 * j + k] = (uint8_t)((lo << 3) | hi);
        }
      }
      T.ntri[t][m] = (uint8_t)nt;
    }
  }
  return T;
}

__constant__ const Table TAB = make_table();

// bit c of the result: corner c of the cell is inside (tsdf < 0); -1 when the cell is not meshed
__device__ __forceinline__ int cell_mask(const Grid& g, int ix, int iy, int iz, int64_t i, const float* __restrict__ tsdf,
                                         const float* __restrict__ weight, float min_weight) {
  if (ix >= g.nx - 1 || iy >= g.ny - 1 || iz >= g.nz - 1) return -1;
  const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
  int mask = 0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int64_t j = i + (c & 1) + ((c >> 1) & 1) * sy + ((c >> 2) & 1) * sz;
    ok = ok && weight[j] >= min_weight;
    mask |= (tsdf[j] < 0.0f ? 1 : 0) << c;
  }
  return ok ? mask : -1;
}

__device__ __forceinline__ int tet_case(const Table& T, int t, int mask) {
  return ((mask >> T.corner[t][0]) & 1) | (((mask >> T.corner[t][1]) & 1) << 1) | (((mask >> T.corner[t][2]) & 1) << 2) |
         (((mask >> T.corner[t][3]) & 1) << 3);
}

__global__ void __launch_bounds__(NT) count_kernel(Grid g, const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                   float min_weight, int32_t* __restrict__ counts) {
  const int64_t plane = (int64_t)g.nx * g.ny * g.nz;
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= plane) return;
  const int ix = (int)(i % g.nx);
  const int64_t r = i / g.nx;
  const int mask = cell_mask(g, ix, (int)(r % g.ny), (int)(r / g.ny), i, tsdf, weight, min_weight);
  int n = 0;
  if (mask > 0 && mask < 255) {
#pragma unroll
    for (int t = 0; t < 6; ++t) n += TAB.ntri[t][tet_case(TAB, t, mask)];
  }
  counts[i] = n;
}

__global__ void __launch_bounds__(NT) emit_kernel(Grid g, const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                  const float* __restrict__ rgb, float min_weight,
                                                  const int32_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                  int64_t n_tri, int64_t* __restrict__ keys, float* __restrict__ pos,
                                                  float* __restrict__ col) {
  const int64_t plane = (int64_t)g.nx * g.ny * g.nz;
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= plane || counts[i] == 0) return;
  const int ix = (int)(i % g.nx);
  const int64_t r = i / g.nx;
  const int iy = (int)(r % g.ny), iz = (int)(r / g.ny);
  const int mask = cell_mask(g, ix, iy, iz, i, tsdf, weight, min_weight);
  if (mask <= 0 || mask >= 255) return;
  const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
  int64_t tri = offsets[i];
  for (int t = 0; t < 6; ++t) {
    const int m = tet_case(TAB, t, mask);
    const int nt = TAB.ntri[t][m];
    for (int j = 0; j < nt; ++j, ++tri) {
      if (tri >= n_tri) return;                           // counts / offsets not of this volume: never write past the buffers
      for (int k = 0; k < 3; ++k) {
        const int e = TAB.edge[t][m][3 * j + k];
        const int a = e >> 3, b = e & 7;
        const int ax = a & 1, ay = (a >> 1) & 1, az = a >> 2, bx = b & 1, by = (b >> 1) & 1, bz = b >> 2;
        const int64_t ia = i + ax + ay * sy + az * sz, ib = i + bx + by * sy + bz * sz;
        const float ta = tsdf[ia], tb = tsdf[ib];
        const float w = ta / (ta - tb);
        const float pax = g.lox + ((float)(ix + ax) + 0.5f) * g.voxel, pbx = g.lox + ((float)(ix + bx) + 0.5f) * g.voxel;
        const float pay = g.loy + ((float)(iy + ay) + 0.5f) * g.voxel, pby = g.loy + ((float)(iy + by) + 0.5f) * g.voxel;
        const float paz = g.loz + ((float)(iz + az) + 0.5f) * g.voxel, pbz = g.loz + ((float)(iz + bz) + 0.5f) * g.voxel;
        const int64_t o = 3 * tri + k;
        keys[o] = ia * 7 + ((a ^ b) - 1);
        pos[3 * o] = pax + (pbx - pax) * w;
        pos[3 * o + 1] = pay + (pby - pay) * w;
        pos[3 * o + 2] = paz + (pbz - paz) * w;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float ca = rgb[c * plane + ia], cb = rgb[c * plane + ib];
          col[3 * o + c] = ca + (cb - ca) * w;
        }
      }
    }
  }
}

// ---- sparse brick volume ------------------------------------------------------------------------------------------------
// The virtual grid is the dense volume's; planes exist only for allocated 8 x 8 x 8 bricks.  table [nbz][nby][nbx] int32: a
// brick's slot or -1.  pool [slot][plane: tsdf, weight, r, g, b][z][y][x] float32, 10 240 B a brick: with a lane per (x, y)
// of a brick layer every access of a wave to a plane is 256 contiguous bytes.  coords [slot][3] int32: (bx, by, bz).
constexpr int BR = 8;
constexpr int BRICK_VOXELS = BR * BR * BR;                     // floats of one plane of a brick
constexpr int BRICK_FLOATS = 5 * BRICK_VOXELS;
static_assert(BR * BR == 64, "a lane per (x, y) of a brick layer");

struct BrickGrid {
  int nbx, nby, nbz;
};

// One WAVE per brick of the virtual grid.  The brick test first; a wave that stays projects its voxels (a lane per (x, y),
// the 8 z layers in two batched passes) and tests them in band: the dense rule would update them and s < 1.  An in-band
// voxel touches its own brick and, on a brick face, the face / edge / corner neighbours inside the grid: 27 bits a lane,
// ORed over the wave; lanes 0..26 then flag the bricks that have no slot yet.  Every writer stores the same value.
__global__ void __launch_bounds__(NT) sparse_mark_kernel(Grid g, Frame f, BrickGrid bg, int64_t nbricks,
                                                         const float4* __restrict__ frame,
                                                         const uint32_t* __restrict__ dmax_bits,
                                                         const int32_t* __restrict__ table, int32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (b >= nbricks) return;                                   // wave-uniform
  const int bx = (int)(b % bg.nbx), by = (int)((b / bg.nbx) % bg.nby), bz = (int)(b / ((int64_t)bg.nbx * bg.nby));
  const int x0 = bx * BR, y0 = by * BR, z0 = bz * BR;
  if (box_outside(g, f, lane, x0, y0, z0, min(x0 + BR, g.nx) - 1, min(y0 + BR, g.ny) - 1, min(z0 + BR, g.nz) - 1, dmax_bits)) return;
  const int lx = lane & 7, ly = lane >> 3;
  const int ix = x0 + lx, iy = y0 + ly;
  const uint32_t mx = 2u | (lx == 0 && ix > 0 ? 1u : 0u) | (lx == BR - 1 && ix + 1 < g.nx ? 4u : 0u);
  const uint32_t my = 2u | (ly == 0 && iy > 0 ? 1u : 0u) | (ly == BR - 1 && iy + 1 < g.ny ? 4u : 0u);
  const uint32_t row = ((my & 1u) ? mx : 0u) | (mx << 3) | ((my & 4u) ? mx << 6 : 0u);
  uint32_t m27 = 0;
#pragma unroll
  for (int pass = 0; pass < BR / PV; ++pass) {
    float zc[PV];
    float4 q[PV];
    bool ok[PV];
#pragma unroll
    for (int v = 0; v < PV; ++v) {
      const int iz = z0 + pass * PV + v;
      int p = 0;
      zc[v] = 0.0f;
      ok[v] = ix < g.nx && iy < g.ny && iz < g.nz && project_voxel(g, f, ix, iy, iz, p, zc[v]);
      q[v] = frame[ok[v] ? p : 0];
    }
#pragma unroll
    for (int v = 0; v < PV; ++v) {
      const int lz = pass * PV + v, iz = z0 + lz;
      float s = 1.0f;
      if (ok[v] && observe(f, q[v].w, zc[v], s) && s < 1.0f) {
        m27 |= row << 9;
        if (lz == 0 && iz > 0) m27 |= row;
        if (lz == BR - 1 && iz + 1 < g.nz) m27 |= row << 18;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m27 |= (uint32_t)__shfl_xor((int)m27, o);
  if (lane < 27 && ((m27 >> lane) & 1u)) {
    const int nx_ = bx + lane % 3 - 1, ny_ = by + (lane / 3) % 3 - 1, nz_ = bz + lane / 9 - 1;
    if (nx_ >= 0 && nx_ < bg.nbx && ny_ >= 0 && ny_ < bg.nby && nz_ >= 0 && nz_ < bg.nbz) {
      const int64_t n = ((int64_t)nz_ * bg.nby + ny_) * bg.nbx + nx_;
      if (table[n] < 0) flags[n] = 1;
    }
  }
}

// flags: 1 for a new brick; offsets: their exclusive scan in brick-linear order.  New brick i gets slot base + offsets[i].
__global__ void __launch_bounds__(NT) sparse_assign_kernel(BrickGrid bg, int64_t nbricks, const int32_t* __restrict__ flags,
                                                           const int64_t* __restrict__ offsets, int64_t base, int64_t n_new,
                                                           int32_t* __restrict__ table, int32_t* __restrict__ coords) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= nbricks || flags[i] == 0) return;
  const int64_t k = offsets[i];
  if (k < 0 || k >= n_new) return;                            // flags / offsets not of this frame: never write past the pool
  const int64_t slot = base + k;
  table[i] = (int32_t)slot;
  coords[3 * slot] = (int32_t)(i % bg.nbx);
  coords[3 * slot + 1] = (int32_t)((i / bg.nbx) % bg.nby);
  coords[3 * slot + 2] = (int32_t)(i / ((int64_t)bg.nbx * bg.nby));
}

__global__ void __launch_bounds__(NT) sparse_fresh_kernel(float4* __restrict__ bricks, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n4) return;
  const float v = (i % (BRICK_FLOATS / 4)) < BRICK_VOXELS / 4 ? 1.0f : 0.0f;            // the tsdf plane comes first
  bricks[i] = make_float4(v, v, v, v);
}

// One WAVE per allocated brick, the walk of integrate_block_kernel: a lane per (x, y), the 8 z layers in passes of PV.
__global__ void __launch_bounds__(NT) sparse_integrate_kernel(Grid g, Frame f, int64_t nslots, const int32_t* __restrict__ coords,
                                                              const float4* __restrict__ frame,
                                                              const uint32_t* __restrict__ dmax_bits, float* __restrict__ pool) {
  const int lane = threadIdx.x & 63;
  const int64_t slot = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (slot >= nslots) return;                                 // wave-uniform
  const int x0 = coords[3 * slot] * BR, y0 = coords[3 * slot + 1] * BR, z0 = coords[3 * slot + 2] * BR;
  if (box_outside(g, f, lane, x0, y0, z0, min(x0 + BR, g.nx) - 1, min(y0 + BR, g.ny) - 1, min(z0 + BR, g.nz) - 1, dmax_bits)) return;
  float* __restrict__ brick = pool + slot * BRICK_FLOATS;
  const int ix = x0 + (lane & 7), iy = y0 + (lane >> 3);
#pragma unroll
  for (int pass = 0; pass < BR / PV; ++pass) {
    int idx[PV];
    float zc[PV], s[PV], w[PV], t[PV], c[PV][3];
    float4 q[PV];
    bool ok[PV];
#pragma unroll
    for (int v = 0; v < PV; ++v) {
      const int lz = pass * PV + v, iz = z0 + lz;
      int p = 0;
      zc[v] = 0.0f;
      ok[v] = ix < g.nx && iy < g.ny && iz < g.nz && project_voxel(g, f, ix, iy, iz, p, zc[v]);
      idx[v] = lz * 64 + lane;
      q[v] = frame[ok[v] ? p : 0];                             // pixel 0 for a voxel that does not project: never used
    }
#pragma unroll
    for (int v = 0; v < PV; ++v) {
      s[v] = 0.0f;
      ok[v] = ok[v] && observe(f, q[v].w, zc[v], s[v]);
      if (ok[v]) {
        t[v] = brick[idx[v]];
        w[v] = brick[BRICK_VOXELS + idx[v]];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[v][k] = brick[(2 + k) * BRICK_VOXELS + idx[v]];
      }
    }
#pragma unroll
    for (int v = 0; v < PV; ++v) {
      if (ok[v]) {
        const float w1 = w[v] + 1.0f;
        brick[idx[v]] = fuse(t[v], w[v], s[v], w1);
        const float o[3] = {q[v].x, q[v].y, q[v].z};
#pragma unroll
        for (int k = 0; k < 3; ++k) brick[(2 + k) * BRICK_VOXELS + idx[v]] = fuse(c[v][k], w[v], o[k], w1);
        brick[BRICK_VOXELS + idx[v]] = fminf(w1, f.max_weight);
      }
    }
  }
}

// The slots of a brick and its 7 upper neighbours (bit 0 = +x, 1 = +y, 2 = +z), looked up once per brick by lanes 0..7 and
// handed to every lane; -1 outside the brick grid or without a slot.  Called by a whole wave.
struct Slots {
  int s[8];
};

__device__ __forceinline__ Slots neighbour_slots(const BrickGrid& bg, const int32_t* __restrict__ table, int lane, int bx, int by,
                                                 int bz) {
  int mine = -1;
  if (lane < 8) {
    const int nx_ = bx + (lane & 1), ny_ = by + ((lane >> 1) & 1), nz_ = bz + (lane >> 2);
    if (nx_ < bg.nbx && ny_ < bg.nby && nz_ < bg.nbz) mine = table[((int64_t)nz_ * bg.nby + ny_) * bg.nbx + nx_];
  }
  Slots r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.s[k] = __shfl(mine, k);
  return r;
}

// offset in the pool of the tsdf of the voxel at brick-local (X, Y, Z) in [0, 16)^3, or -1 when its brick has no slot
__device__ __forceinline__ int64_t voxel_offset(const Slots& n, int X, int Y, int Z) {
  const bool xb = X >= BR, yb = Y >= BR, zb = Z >= BR;
  const int a0 = xb ? n.s[1] : n.s[0], a1 = xb ? n.s[3] : n.s[2], a2 = xb ? n.s[5] : n.s[4], a3 = xb ? n.s[7] : n.s[6];
  const int b0 = yb ? a1 : a0, b1 = yb ? a3 : a2;
  const int slot = zb ? b1 : b0;
  if (slot < 0) return -1;
  return (int64_t)slot * BRICK_FLOATS + ((Z & 7) * 64 + (Y & 7) * 8 + (X & 7));
}

// cell_mask on the brick pool: an unallocated corner has weight 0 and tsdf 1
__device__ __forceinline__ int sparse_cell_mask(const Grid& g, const Slots& n, int ix, int iy, int iz, int lx, int ly, int lz,
                                                const float* __restrict__ pool, float min_weight) {
  if (ix >= g.nx - 1 || iy >= g.ny - 1 || iz >= g.nz - 1) return -1;
  int mask = 0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int64_t o = voxel_offset(n, lx + (c & 1), ly + ((c >> 1) & 1), lz + (c >> 2));
    const float w = o >= 0 ? pool[o + BRICK_VOXELS] : 0.0f;
    const float t = o >= 0 ? pool[o] : 1.0f;
    ok = ok && w >= min_weight;
    mask |= (t < 0.0f ? 1 : 0) << c;
  }
  return ok ? mask : -1;
}

// One WAVE per allocated brick: counts [slot][z][y][x] of the cells whose lower corner lies in the brick.
__global__ void __launch_bounds__(NT) sparse_count_kernel(Grid g, BrickGrid bg, int64_t nslots, const int32_t* __restrict__ coords,
                                                          const int32_t* __restrict__ table, const float* __restrict__ pool,
                                                          float min_weight, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t slot = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (slot >= nslots) return;                                 // wave-uniform
  const int bx = coords[3 * slot], by = coords[3 * slot + 1], bz = coords[3 * slot + 2];
  const Slots n = neighbour_slots(bg, table, lane, bx, by, bz);
  const int lx = lane & 7, ly = lane >> 3;
  const int ix = bx * BR + lx, iy = by * BR + ly;
  for (int lz = 0; lz < BR; ++lz) {
    const int iz = bz * BR + lz;
    int cnt = 0;
    if (ix < g.nx && iy < g.ny && iz < g.nz) {
      const int mask = sparse_cell_mask(g, n, ix, iy, iz, lx, ly, lz, pool, min_weight);
      if (mask > 0 && mask < 255) {
#pragma unroll
        for (int t = 0; t < 6; ++t) cnt += TAB.ntri[t][tet_case(TAB, t, mask)];
      }
    }
    counts[slot * BRICK_VOXELS + lz * 64 + lane] = cnt;
  }
}

// emit_kernel on the brick pool; cells [n_tri]: the virtual linear index of every triangle's cell, for the caller's stable
// sort into virtual-cell order (bricks leave in slot order).
__global__ void __launch_bounds__(NT) sparse_emit_kernel(Grid g, BrickGrid bg, int64_t nslots, const int32_t* __restrict__ coords,
                                                         const int32_t* __restrict__ table, const float* __restrict__ pool,
                                                         float min_weight, const int32_t* __restrict__ counts,
                                                         const int64_t* __restrict__ offsets, int64_t n_tri,
                                                         int64_t* __restrict__ cells, int64_t* __restrict__ keys,
                                                         float* __restrict__ pos, float* __restrict__ col) {
  const int lane = threadIdx.x & 63;
  const int64_t slot = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (slot >= nslots) return;                                 // wave-uniform
  const int bx = coords[3 * slot], by = coords[3 * slot + 1], bz = coords[3 * slot + 2];
  const Slots n = neighbour_slots(bg, table, lane, bx, by, bz);
  const int lx = lane & 7, ly = lane >> 3;
  const int ix = bx * BR + lx, iy = by * BR + ly;
  const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
  for (int lz = 0; lz < BR; ++lz) {
    const int iz = bz * BR + lz;
    const int64_t cslot = slot * BRICK_VOXELS + lz * 64 + lane;
    if (!(ix < g.nx && iy < g.ny && iz < g.nz) || counts[cslot] == 0) continue;
    const int mask = sparse_cell_mask(g, n, ix, iy, iz, lx, ly, lz, pool, min_weight);
    if (mask <= 0 || mask >= 255) continue;
    const int64_t i = ((int64_t)iz * g.ny + iy) * g.nx + ix;
    int64_t tri = offsets[cslot];
    for (int t = 0; t < 6; ++t) {
      const int m = tet_case(TAB, t, mask);
      const int nt = TAB.ntri[t][m];
      for (int j = 0; j < nt; ++j, ++tri) {
        if (tri >= n_tri) return;                           // counts / offsets not of this volume: never write past the buffers
        cells[tri] = i;
        for (int k = 0; k < 3; ++k) {
          const int e = TAB.edge[t][m][3 * j + k];
          const int a = e >> 3, b = e & 7;
          const int ax = a & 1, ay = (a >> 1) & 1, az = a >> 2, bx_ = b & 1, by_ = (b >> 1) & 1, bz_ = b >> 2;
          const int64_t ia = i + ax + ay * sy + az * sz;
          const int64_t oa = voxel_offset(n, lx + ax, ly + ay, lz + az), ob = voxel_offset(n, lx + bx_, ly + by_, lz + bz_);
          if (oa < 0 || ob < 0) return;                     // a meshed cell has all 8 corners allocated (min_weight > 0)
          const float ta = pool[oa], tb = pool[ob];
          const float w = ta / (ta - tb);
          const float pax = g.lox + ((float)(ix + ax) + 0.5f) * g.voxel, pbx = g.lox + ((float)(ix + bx_) + 0.5f) * g.voxel;
          const float pay = g.loy + ((float)(iy + ay) + 0.5f) * g.voxel, pby = g.loy + ((float)(iy + by_) + 0.5f) * g.voxel;
          const float paz = g.loz + ((float)(iz + az) + 0.5f) * g.voxel, pbz = g.loz + ((float)(iz + bz_) + 0.5f) * g.voxel;
          const int64_t o = 3 * tri + k;
          keys[o] = ia * 7 + ((a ^ b) - 1);
          pos[3 * o] = pax + (pbx - pax) * w;
          pos[3 * o + 1] = pay + (pby - pay) * w;
          pos[3 * o + 2] = paz + (pbz - paz) * w;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float ca = pool[oa + (2 + c) * BRICK_VOXELS], cb = pool[ob + (2 + c) * BRICK_VOXELS];
            col[3 * o + c] = ca + (cb - ca) * w;
          }
        }
      }
    }
  }
}

// the box [x0, x0 + wx) x [y0, y0 + wy) x [z0, z0 + wz) of the virtual grid as dense planes; unallocated bricks read fresh
__global__ void __launch_bounds__(NT) sparse_to_dense_kernel(BrickGrid bg, const int32_t* __restrict__ table,
                                                             const float* __restrict__ pool, int x0, int y0, int z0, int wx, int wy,
                                                             int64_t n, float* __restrict__ tsdf, float* __restrict__ weight,
                                                             float* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int ix = x0 + (int)(i % wx);
  const int64_t r = i / wx;
  const int iy = y0 + (int)(r % wy), iz = z0 + (int)(r / wy);
  const int slot = table[((int64_t)(iz >> 3) * bg.nby + (iy >> 3)) * bg.nbx + (ix >> 3)];
  float v[5] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (slot >= 0) {
    const float* __restrict__ p = pool + (int64_t)slot * BRICK_FLOATS + ((iz & 7) * 64 + (iy & 7) * 8 + (ix & 7));
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = p[k * BRICK_VOXELS];
  }
  tsdf[i] = v[0];
  weight[i] = v[1];
#pragma unroll
  for (int k = 0; k < 3; ++k) rgb[k * n + i] = v[2 + k];
}

static int g_dense = -1;

static bool dense_form() {
  if (g_dense < 0) {
    const char* e = getenv("RTGS_TSDF_DENSE");
    g_dense = (e && e[0] == '1') ? 1 : 0;
  }
  return g_dense == 1;
}

static bool grid_ok(int nx, int ny, int nz, float voxel) {
  return nx >= 1 && ny >= 1 && nz >= 1 && voxel > 0.0f && (int64_t)nx * ny * nz <= RTGS_TSDF_MAX_VOXELS;
}

static Frame make_frame(const float* lo3_host, int nx, int ny, int nz, float voxel, float trunc, float max_weight, int H, int W,
                        float fx, float fy, float cx, float cy, const float* w2c12_host) {
  Frame f;
  for (int i = 0; i < 9; ++i) f.r[i] = w2c12_host[i];
  for (int i = 0; i < 3; ++i) f.t[i] = w2c12_host[9 + i];
  f.fx = fx; f.fy = fy; f.cx = cx; f.cy = cy; f.H = H; f.W = W; f.trunc = trunc; f.max_weight = max_weight;
  // largest magnitude a camera-space coordinate can reach over the volume's voxel centres, per row
  double ext[3];
  const int n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) {
    const double l = lo3_host[a], h = l + (double)n[a] * voxel;
    ext[a] = fabs(l) > fabs(h) ? fabs(l) : fabs(h);
  }
  double B[3];
  for (int row = 0; row < 3; ++row)
    B[row] = fabs(f.r[3 * row]) * ext[0] + fabs(f.r[3 * row + 1]) * ext[1] + fabs(f.r[3 * row + 2]) * ext[2] + fabs(f.t[row]);
  const double rel = 2e-5;                                 // ~170 ulp of float32: the chain has fewer than 16 roundings
  f.mz = (float)(rel * (B[2] + trunc) + 1e-30);
  f.mx = (float)(rel * (fabs(fx) * B[0] + (fabs(cx) + W + 1.0) * B[2]) + 1e-30);
  f.my = (float)(rel * (fabs(fy) * B[1] + (fabs(cy) + H + 1.0) * B[2]) + 1e-30);
  return f;
}

static bool sparse_grid_ok(int nx, int ny, int nz, float voxel) {
  const int lim = 1 << 24;                                   // (float)i is exact
  if (!(nx >= 1 && ny >= 1 && nz >= 1 && nx <= lim && ny <= lim && nz <= lim && voxel > 0.0f)) return false;
  return (int64_t)((nx + BR - 1) / BR) * ((ny + BR - 1) / BR) * ((nz + BR - 1) / BR) <= RTGS_TSDF_SPARSE_MAX_BRICKS;
}

static BrickGrid brick_grid(int nx, int ny, int nz) { return BrickGrid{(nx + BR - 1) / BR, (ny + BR - 1) / BR, (nz + BR - 1) / BR}; }

static bool frame_args_ok(float trunc, float max_weight, int H, int W) {
  return trunc > 0.0f && max_weight >= 1.0f && H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffffLL;
}

// launch of one wave per item, WAVES waves a group; false when the grid would not fit
static bool wave_groups(int64_t items, unsigned& groups) {
  const int64_t n = (items + WAVES - 1) / WAVES;
  if (n > 0x7fffffffLL) return false;
  groups = (unsigned)n;
  return true;
}

}  // namespace rtgs_tsdf

extern "C" {

void rtgs_tsdf_set_dense(int on) { rtgs_tsdf::g_dense = on ? 1 : 0; }

size_t rtgs_tsdf_scratch_bytes(int32_t H, int32_t W) {
  return H > 0 && W > 0 ? 16 + (size_t)H * (size_t)W * sizeof(float4) : 0;
}

int rtgs_tsdf_integrate(float* tsdf, float* weight, float* rgb, int32_t nx, int32_t ny, int32_t nz, const float* lo3_host,
                        float voxel, float trunc, float max_weight, const float* depth, const float* color, int32_t H, int32_t W,
                        float fx, float fy, float cx, float cy, const float* w2c12_host, void* scratch, void* stream) {
  using namespace rtgs_tsdf;
  if (!tsdf || !weight || !rgb || !lo3_host || !depth || !color || !w2c12_host || !scratch) return -1;
  if (!grid_ok(nx, ny, nz, voxel) || !(trunc > 0.0f) || !(max_weight >= 1.0f) || H <= 0 || W <= 0 ||
      (int64_t)H * W > 0x7fffffffLL)
    return -1;
  const Grid g{nx, ny, nz, lo3_host[0], lo3_host[1], lo3_host[2], voxel};
  const Frame f = make_frame(lo3_host, nx, ny, nz, voxel, trunc, max_weight, H, W, fx, fy, cx, cy, w2c12_host);
  hipStream_t s = (hipStream_t)stream;
  const int64_t plane = (int64_t)nx * ny * nz;
  if (((uintptr_t)scratch & 15u) != 0) return -1;
  uint32_t* dmax = (uint32_t*)scratch;
  float4* frame = (float4*)((char*)scratch + 16);
  if (hipMemsetAsync(dmax, 0, sizeof(uint32_t), s) != hipSuccess) return -2;
  const int64_t npix = (int64_t)H * W;
  const int64_t rb = (npix + NT - 1) / NT;
  hipLaunchKernelGGL(pack_frame_kernel, dim3((unsigned)(rb < PACK_GROUPS ? rb : PACK_GROUPS)), dim3(NT), 0, s, depth, color, npix,
                     frame, dmax);
  if (dense_form()) {
    hipLaunchKernelGGL(integrate_dense_kernel, dim3((unsigned)((plane + NT - 1) / NT)), dim3(NT), 0, s, g, f, frame, tsdf,
                       weight, rgb);
  } else {
    const int nbx = (nx + BX - 1) / BX, nby = (ny + BY - 1) / BY, nbz = (nz + BZ - 1) / BZ;
    const int64_t blocks = (int64_t)nbx * nby * nbz;
    const int64_t groups = (blocks + WAVES - 1) / WAVES;
    if (groups > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(integrate_block_kernel, dim3((unsigned)groups), dim3(NT), 0, s, g, f, nbx, nby, blocks, frame, dmax, tsdf,
                       weight, rgb);
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_tsdf_count(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float min_weight,
                    int32_t* counts, void* stream) {
  using namespace rtgs_tsdf;
  if (!tsdf || !weight || !counts || !grid_ok(nx, ny, nz, 1.0f)) return -1;
  const Grid g{nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f};
  const int64_t plane = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(count_kernel, dim3((unsigned)((plane + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, g, tsdf, weight,
                     min_weight, counts);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_tsdf_emit(const float* tsdf, const float* weight, const float* rgb, int32_t nx, int32_t ny, int32_t nz,
                   const float* lo3_host, float voxel, float min_weight, const int32_t* counts, const int64_t* offsets,
                   int64_t n_tri, int64_t* keys, float* positions, float* colors, void* stream) {
  using namespace rtgs_tsdf;
  if (n_tri == 0) return 0;
  if (!tsdf || !weight || !rgb || !lo3_host || !counts || !offsets || !keys || !positions || !colors || n_tri < 0 ||
      !grid_ok(nx, ny, nz, voxel))
    return -1;
  const Grid g{nx, ny, nz, lo3_host[0], lo3_host[1], lo3_host[2], voxel};
  const int64_t plane = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(emit_kernel, dim3((unsigned)((plane + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, g, tsdf, weight, rgb,
                     min_weight, counts, offsets, n_tri, keys, positions, colors);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_tsdf_sparse_mark(const int32_t* table, int32_t* flags, int32_t nx, int32_t ny, int32_t nz, const float* lo3_host,
                          float voxel, float trunc, const float* depth, const float* color, int32_t H, int32_t W, float fx, float fy,
                          float cx, float cy, const float* w2c12_host, void* scratch, void* stream) {
  using namespace rtgs_tsdf;
  if (!table || !flags || !lo3_host || !depth || !color || !w2c12_host || !scratch || ((uintptr_t)scratch & 15u) != 0) return -1;
  if (!sparse_grid_ok(nx, ny, nz, voxel) || !frame_args_ok(trunc, 1.0f, H, W)) return -1;
  const Grid g{nx, ny, nz, lo3_host[0], lo3_host[1], lo3_host[2], voxel};
  const Frame f = make_frame(lo3_host, nx, ny, nz, voxel, trunc, 1.0f, H, W, fx, fy, cx, cy, w2c12_host);
  const BrickGrid bg = brick_grid(nx, ny, nz);
  const int64_t nbricks = (int64_t)bg.nbx * bg.nby * bg.nbz;
  unsigned groups;
  if (!wave_groups(nbricks, groups)) return -1;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* dmax = (uint32_t*)scratch;
  float4* frame = (float4*)((char*)scratch + 16);
  if (hipMemsetAsync(dmax, 0, sizeof(uint32_t), s) != hipSuccess) return -2;
  if (hipMemsetAsync(flags, 0, (size_t)nbricks * sizeof(int32_t), s) != hipSuccess) return -2;
  const int64_t npix = (int64_t)H * W;
  const int64_t rb = (npix + NT - 1) / NT;
  hipLaunchKernelGGL(pack_frame_kernel, dim3((unsigned)(rb < PACK_GROUPS ? rb : PACK_GROUPS)), dim3(NT), 0, s, depth, color, npix,
                     frame, dmax);
  hipLaunchKernelGGL(sparse_mark_kernel, dim3(groups), dim3(NT), 0, s, g, f, bg, nbricks, frame, dmax, table, flags);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_tsdf_sparse_allocate(int32_t* table, const int32_t* flags, const int64_t* offsets, int32_t nx, int32_t ny, int32_t nz,
                              int64_t base, int64_t n_new, int64_t capacity, int32_t* coords, float* pool, void* stream) {
  using namespace rtgs_tsdf;
  if (n_new == 0) return 0;
  if (!table || !flags || !offsets || !coords || !pool || ((uintptr_t)pool & 15u) != 0 || !sparse_grid_ok(nx, ny, nz, 1.0f)) return -1;
  if (base < 0 || n_new < 0 || base + n_new > capacity || capacity > RTGS_TSDF_SPARSE_MAX_BRICKS) return -1;
  const BrickGrid bg = brick_grid(nx, ny, nz);
  const int64_t nbricks = (int64_t)bg.nbx * bg.nby * bg.nbz;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sparse_assign_kernel, dim3((unsigned)((nbricks + NT - 1) / NT)), dim3(NT), 0, s, bg, nbricks, flags, offsets,
                     base, n_new, table, coords);
  const int64_t n4 = n_new * (BRICK_FLOATS / 4);
  if ((n4 + NT - 1) / NT > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(sparse_fresh_kernel, dim3((unsigned)((n4 + NT - 1) / NT)), dim3(NT), 0, s,
                     (float4*)(pool + base * BRICK_FLOATS), n4);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_tsdf_sparse_integrate(float* pool, const int32_t* coords, int64_t n_bricks, int32_t nx, int32_t ny, int32_t nz,
                               const float* lo3_host, float voxel, float trunc, float max_weight, int32_t H, int32_t W, float fx,
                               float fy, float cx, float cy, const float* w2c12_host, const void* scratch, void* stream) {
  using namespace rtgs_tsdf;
  if (n_bricks == 0) return 0;
  if (!pool || !coords || !lo3_host || !w2c12_host || !scratch || ((uintptr_t)scratch & 15u) != 0) return -1;
  if (n_bricks < 0 || n_bricks > RTGS_TSDF_SPARSE_MAX_BRICKS || !sparse_grid_ok(nx, ny, nz, voxel) ||
      !frame_args_ok(trunc, max_weight, H, W))
    return -1;
  const Grid g{nx, ny, nz, lo3_host[0], lo3_host[1], lo3_host[2], voxel};
  const Frame f = make_frame(lo3_host, nx, ny, nz, voxel, trunc, max_weight, H, W, fx, fy, cx, cy, w2c12_host);
  unsigned groups;
  if (!wave_groups(n_bricks, groups)) return -1;
  hipLaunchKernelGGL(sparse_integrate_kernel, dim3(groups), dim3(NT), 0, (hipStream_t)stream, g, f, n_bricks, coords,
                     (const float4*)((const char*)scratch + 16), (const uint32_t*)scratch, pool);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_tsdf_sparse_count(const float* pool, const int32_t* coords, const int32_t* table, int64_t n_bricks, int32_t nx,
                           int32_t ny, int32_t nz, float min_weight, int32_t* counts, void* stream) {
  using namespace rtgs_tsdf;
  if (n_bricks == 0) return 0;
  if (!pool || !coords || !table || !counts || n_bricks < 0 || n_bricks > RTGS_TSDF_SPARSE_MAX_BRICKS ||
      !sparse_grid_ok(nx, ny, nz, 1.0f) || !(min_weight > 0.0f))
    return -1;
  const Grid g{nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f};
  unsigned groups;
  if (!wave_groups(n_bricks, groups)) return -1;
  hipLaunchKernelGGL(sparse_count_kernel, dim3(groups), dim3(NT), 0, (hipStream_t)stream, g, brick_grid(nx, ny, nz), n_bricks,
                     coords, table, pool, min_weight, counts);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_tsdf_sparse_emit(const float* pool, const int32_t* coords, const int32_t* table, int64_t n_bricks, int32_t nx, int32_t ny,
                          int32_t nz, const float* lo3_host, float voxel, float min_weight, const int32_t* counts,
                          const int64_t* offsets, int64_t n_tri, int64_t* cells, int64_t* keys, float* positions, float* colors,
                          void* stream) {
  using namespace rtgs_tsdf;
  if (n_tri == 0 || n_bricks == 0) return 0;
  if (!pool || !coords || !table || !lo3_host || !counts || !offsets || !cells || !keys || !positions || !colors || n_tri < 0 ||
      n_bricks < 0 || n_bricks > RTGS_TSDF_SPARSE_MAX_BRICKS || !sparse_grid_ok(nx, ny, nz, voxel) || !(min_weight > 0.0f))
    return -1;
  const Grid g{nx, ny, nz, lo3_host[0], lo3_host[1], lo3_host[2], voxel};
  unsigned groups;
  if (!wave_groups(n_bricks, groups)) return -1;
  hipLaunchKernelGGL(sparse_emit_kernel, dim3(groups), dim3(NT), 0, (hipStream_t)stream, g, brick_grid(nx, ny, nz), n_bricks,
                     coords, table, pool, min_weight, counts, offsets, n_tri, cells, keys, positions, colors);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_tsdf_sparse_to_dense(const float* pool, const int32_t* table, int32_t nx, int32_t ny, int32_t nz, const int32_t* window6_host,
                              float* tsdf, float* weight, float* rgb, void* stream) {
  using namespace rtgs_tsdf;
  if (!pool || !table || !window6_host || !tsdf || !weight || !rgb || !sparse_grid_ok(nx, ny, nz, 1.0f)) return -1;
  const int32_t* w = window6_host;
  if (w[0] < 0 || w[1] <= w[0] || w[1] > nx || w[2] < 0 || w[3] <= w[2] || w[3] > ny || w[4] < 0 || w[5] <= w[4] || w[5] > nz)
    return -1;
  const int wx = w[1] - w[0], wy = w[3] - w[2], wz = w[5] - w[4];
  const int64_t n = (int64_t)wx * wy * wz;
  if ((n + NT - 1) / NT > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(sparse_to_dense_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream,
                     brick_grid(nx, ny, nz), table, pool, w[0], w[2], w[4], wx, wy, n, tsdf, weight, rgb);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
