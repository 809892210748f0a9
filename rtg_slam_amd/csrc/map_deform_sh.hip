// rtgs_map_deform_sh (include/rtgs_slam.h): the higher SH bands turn with the deformed map.  Behind rtgs_map_deform, every row
// whose frame's correction rotates gets its bands 1..3 multiplied, channel by channel, by the three matrices of that rotation
// (rtg_slam_amd/sh_rotation.py builds them on the host).  No atomics, no host read; tests/map_deform_sh_reference.py restates the
// float32 chain below and the kernel matches it bit for bit (fmaf is written out, the file is built with -ffp-contract=off).
//
// A block of three waves takes 64 rows.  A row is 192 B, so one lane per row would read with a 192-B stride; instead
//   1  wave 0 reads the 64 ticks, clamps them and reads each frame's flag; LDS keeps the frame, or -1 for a row that stays;
//   2  all lanes copy the moved rows into LDS, one float4 per lane and load (12 per row, 1 KiB per wave instruction), at a row
//      stride of 49 floats;
//   3  wave c turns channel c: lane r reads its 15 values of row r (stride 49 floats: the 32 lanes of a half wave hit 32 banks),
//      multiplies and writes them back to the same slots, which no other lane touches;
//   4  all lanes copy the rows back, float4 again.  A row's first float4 holds the DC term and one coefficient of band 1: only
//      that one float is stored.  A row that stays is neither loaded nor stored; a block of such rows ends after step 1.
// The matrix: rows added by one frame lie next to each other, so most waves need ONE table row - its 83 values then come through
// scalar loads and sit in SGPRs (the FMA takes them as they are).  A wave whose moved rows differ in their frame gathers the values
// per lane.  Both paths run the same chain.
//
// Traffic per moved row: 192 B in (the DC term comes along with its float4), 180 B out, the tick, and the 336-B table row from
// the cache.  LDS: 64 x 49 x 4 B + 256 B = 12.5 KiB a block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtgs_slam.h"

namespace rtgs {

constexpr int kShRows = 64;         // rows per block = lanes per wave
constexpr int kShThreads = 192;     // one wave per colour channel
constexpr int kShStride = 49;       // floats between two rows in LDS: odd, so that lane r -> bank (17 r + const) % 32 is one to one
constexpr int kShTable = 84;        // floats per table row: 9 + 25 + 49 matrix values, the flag

// out[i] = sum_j M[i][j] x[j] in the definition's order: the last product first, then fmaf down to j = 0
template <int n>
__device__ __forceinline__ void sh_band(const float* __restrict__ M, const float* x, float* out) {
#pragma unroll
  for (int i = 0; i < n; ++i) {
    float acc = M[i * n + n - 1] * x[n - 1];
#pragma unroll
    for (int j = n - 2; j >= 0; --j) acc = fmaf(M[i * n + j], x[j], acc);
    out[i] = acc;
  }
}

// x = coefficients 1..15 of one channel, turned in place
__device__ __forceinline__ void sh_turn(const float* __restrict__ M, float* x) {
  float o[15];
  sh_band<3>(M, x, o);
  sh_band<5>(M + 9, x + 3, o + 3);
  sh_band<7>(M + 34, x + 8, o + 8);
#pragma unroll
  for (int k = 0; k < 15; ++k) x[k] = o[k];
}

template <typename TickT>
__global__ void __launch_bounds__(kShThreads) map_deform_sh_kernel(float* __restrict__ shs, const TickT* __restrict__ tick, long long N,
                                                                   const float* __restrict__ table, int n_frames) {
  __shared__ float s_row[kShRows * kShStride];
  __shared__ int s_frame[kShRows];
  const int t = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * kShRows;
  if (t < kShRows) {
    int frame = -1;
    if (row0 + t < N) {
      long long f = (long long)tick[row0 + t];
      f = f < 0 ? 0 : (f > (long long)n_frames - 1 ? (long long)n_frames - 1 : f);
      if (!(table[f * kShTable + kShTable - 1] == 0.0f)) frame = (int)f;
    }
    s_frame[t] = frame;
  }
  // the block's verdict rides on the barrier: no row moved, nothing to do
  if (!__syncthreads_or(t < kShRows && s_frame[t] >= 0)) return;

  float4* __restrict__ rows4 = (float4*)shs + row0 * 12;
  float4 v[4];
  bool on[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {                                // the four loads leave before the first is waited for
    const int e = t + k * kShThreads;
    on[k] = s_frame[e / 12] >= 0;
    if (on[k]) v[k] = rows4[e];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int e = t + k * kShThreads, r = e / 12, q = e - 12 * r;
    if (on[k]) {
      float* d = s_row + r * kShStride + 4 * q;
      d[0] = v[k].x; d[1] = v[k].y; d[2] = v[k].z; d[3] = v[k].w;
    }
  }
  __syncthreads();

  {
    const int lane = t & 63, c = t >> 6;
    const int frame = s_frame[lane];
    const bool moved = frame >= 0;
    const unsigned long long mask = __ballot(moved);
    if (mask != 0ull) {
      const int shared_frame = __builtin_amdgcn_readfirstlane(s_frame[__ffsll((long long)mask) - 1]);   // the first moved row's
      float* mine = s_row + lane * kShStride + 3 + c;
      float x[15];
      if (__all(!moved || frame == shared_frame)) {           // the same branch in every lane: the table row goes through SGPRs
        if (moved) {
#pragma unroll
          for (int k = 0; k < 15; ++k) x[k] = mine[3 * k];
          sh_turn((const float*)__builtin_assume_aligned(table + (long long)shared_frame * kShTable, 16), x);
#pragma unroll
          for (int k = 0; k < 15; ++k) mine[3 * k] = x[k];
        }
      } else if (moved) {
#pragma unroll
        for (int k = 0; k < 15; ++k) x[k] = mine[3 * k];
        sh_turn((const float*)__builtin_assume_aligned(table + (long long)frame * kShTable, 16), x);
#pragma unroll
        for (int k = 0; k < 15; ++k) mine[3 * k] = x[k];
      }
    }
  }
  __syncthreads();

#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int e = t + k * kShThreads, r = e / 12, q = e - 12 * r;
    if (s_frame[r] >= 0) {
      const float* d = s_row + r * kShStride + 4 * q;
      if (q == 0)
        shs[(row0 + r) * 48 + 3] = d[3];                       // coefficient 0 is never written
      else
        rows4[e] = make_float4(d[0], d[1], d[2], d[3]);
    }
  }
}

}  // namespace rtgs

extern "C" int rtgs_map_deform_sh(float* shs, const void* tick, int32_t tick_kind, int64_t N, const float* sh_table, int32_t n_frames,
                                  void* stream) {
  if (N < 0 || N > RTGS_MAP_DEFORM_MAX_ROWS || n_frames < 1 || (tick_kind != 0 && tick_kind != 1)) return -1;
  if (N == 0) return 0;
  if (!shs || !tick || !sh_table) return -1;
  if (((uintptr_t)shs & 15) || ((uintptr_t)sh_table & 15)) return -1;
  const dim3 grid((unsigned)((N + rtgs::kShRows - 1) / rtgs::kShRows)), block(rtgs::kShThreads);
  if (tick_kind == 0)
    hipLaunchKernelGGL(rtgs::map_deform_sh_kernel<int32_t>, grid, block, 0, (hipStream_t)stream, shs, (const int32_t*)tick, (long long)N,
                       sh_table, (int)n_frames);
  else
    hipLaunchKernelGGL(rtgs::map_deform_sh_kernel<int64_t>, grid, block, 0, (hipStream_t)stream, shs, (const int64_t*)tick, (long long)N,
                       sh_table, (int)n_frames);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
