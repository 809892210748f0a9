// rtgs_keypoint_detect / rtgs_keypoint_describe / rtgs_keypoint_match (include/rtgs_slam.h): corners, binary descriptors and a
// brute-force Hamming match for the loop closure's wide-baseline revisits.  tests/keypoint_reference.py is the definition; after
// the grey value everything is integer arithmetic, so order does not matter and the kernels match it bit for bit.
//
// detect: one block of 256 threads per cell of c x c pixels (8 <= c <= 32).  The cell's g8 with a halo of 4 (1 for the 3 x 3
//   non-maximum suppression + 3 for the circle; box5's 2 lie within) is staged in LDS as bytes, out-of-image pixels as 0; from it
//   come the cell's g8 and box5 planes, then the eligible FAST-9 scores of the cell plus a halo of 1 (each computed once per cell,
//   into LDS), then the suppression and the cell's maximum as one packed key (score << 16 | 0xFFFF - row-major index in the cell):
//   a wave shuffle, then four keys through LDS.  LDS: 40 x 40 B + 34 x 34 x 4 B + 16 B = 6 240 B.
// describe: one wave per slot, four per block.  The two moments are int32 sums over the disc's 529 pixels (at most 13 x 255 x 529
//   < 2^31), reduced by butterflies; the 32 directions are scored in int64 by lanes 0 .. 31 and reduced with the tie rule; the
//   256 tests run as four rounds of 64, a ballot packs each round into two words.
// match: blockIdx.y is the (query set, reference set) pair, one wave per query, four queries per block; the block stages the
//   reference descriptors through LDS in tiles of 256 (8 KiB, word-major: lane l reads word w of reference j at [w][j], no bank
//   conflict), lane l takes references l, l + 64, ... of a tile, and the wave merges (best, index, second) by butterflies.
// No atomics, no host read; nothing here depends on the order in which blocks or waves run.  Compiled with -ffp-contract=off:
// the grey value's float32 chain is part of the definition.
#include "keypoint_common.h"

namespace rtgs {

constexpr int KP_TILE = 256;
constexpr int KP_NONE = 257;

// the cell's body is detect_cell, the slot's describe_slot (keypoint_common.h): csrc/keypoint_pyramid.hip runs the same two over
// the levels of a pyramid
__global__ void __launch_bounds__(KP_THREADS) keypoint_detect_kernel(const float* __restrict__ color, const float* __restrict__ depth, int H, int W,
                                                                      int c, int ncx, int threshold, uint8_t* __restrict__ g8_out,
                                                                      int32_t* __restrict__ box_out, int32_t* __restrict__ slots) {
  detect_cell(GreyOfColor{color, (long long)H * W}, depth, H, W, c, (int)blockIdx.x, (int)blockIdx.y, threshold, g8_out, box_out,
              slots + 4 * ((long long)blockIdx.y * ncx + blockIdx.x));
}

__global__ void __launch_bounds__(KP_THREADS) keypoint_describe_kernel(const uint8_t* __restrict__ g8, const int32_t* __restrict__ box, int H, int W,
                                                                        int ncells, int oriented, const int32_t* __restrict__ dirs,
                                                                        const uint32_t* __restrict__ tables, int32_t* __restrict__ slots,
                                                                        uint32_t* __restrict__ desc) {
  const int lane = threadIdx.x & (KP_WAVE - 1);
  const int slot = (int)blockIdx.x * KP_WAVES + (threadIdx.x >> 6);
  if (slot >= ncells) return;                                      // wave-uniform: the shuffles of describe_slot see whole waves
  describe_slot(g8, box, H, W, oriented, dirs, tables, slots + 4 * (long long)slot, desc + 8 * (long long)slot, lane);
}

__global__ void __launch_bounds__(KP_THREADS) keypoint_match_kernel(const uint32_t* __restrict__ desc, long long n_desc, const int32_t* __restrict__ pairs,
                                                                     long long n_out, int32_t* __restrict__ out) {
  __shared__ uint32_t tile[8][KP_TILE];
  const int tid = threadIdx.x, lane = tid & (KP_WAVE - 1), wave = tid >> 6;
  const int32_t* p = pairs + 5 * (long long)blockIdx.y;
  const long long qb = p[0], qn = p[1], rb = p[2], rn = p[3], ob = p[4];
  // block-uniform exits, before any barrier: a table that points outside the buffers is not followed
  if (qb < 0 || qn < 0 || rb < 0 || rn < 0 || ob < 0 || qb + qn > n_desc || rb + rn > n_desc || ob + qn > n_out) return;
  const long long q0 = (long long)blockIdx.x * KP_WAVES;
  if (q0 >= qn) return;
  const long long q = q0 + wave;
  const bool live = q < qn;
  uint32_t qd[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) qd[w] = live ? desc[8 * (qb + q) + w] : 0u;
  int best = KP_NONE, idx = INT_MAX, second = KP_NONE;
  for (long long t0 = 0; t0 < rn; t0 += KP_TILE) {
    __syncthreads();                                               // the tile before this one has been read by every wave
    if (t0 + tid < rn) {
      const uint4* src = reinterpret_cast<const uint4*>(desc + 8 * (rb + t0 + tid));
      const uint4 a = src[0], b = src[1];
      tile[0][tid] = a.x;
      tile[1][tid] = a.y;
      tile[2][tid] = a.z;
      tile[3][tid] = a.w;
      tile[4][tid] = b.x;
      tile[5][tid] = b.y;
      tile[6][tid] = b.z;
      tile[7][tid] = b.w;
    }
    __syncthreads();
    if (live) {
      const int n = (int)(rn - t0 < KP_TILE ? rn - t0 : KP_TILE);
      for (int j = lane; j < n; j += KP_WAVE) {                    // ascending indices per lane: a strict < keeps the lowest
        int d = 0;
#pragma unroll
        for (int w = 0; w < 8; ++w) d += __popc(qd[w] ^ tile[w][j]);
        if (d < best) {
          second = best;
          best = d;
          idx = (int)(t0 + j);
        } else if (d < second) {
          second = d;
        }
      }
    }
  }
  if (!live) return;                                               // wave-uniform
  for (int o = KP_WAVE / 2; o >= 1; o >>= 1) {                     // the two sides of every step hold disjoint reference sets
    const int ob_ = __shfl_xor(best, o, KP_WAVE), oi = __shfl_xor(idx, o, KP_WAVE), os = __shfl_xor(second, o, KP_WAVE);
    const bool other = ob_ < best || (ob_ == best && oi < idx);
    const int loser = other ? best : ob_;
    if (other) {
      best = ob_;
      idx = oi;
    }
    second = min(min(second, os), loser);
  }
  if (lane == 0) {
    int32_t* o3 = out + 3 * (ob + q);
    o3[0] = idx == INT_MAX ? -1 : idx;
    o3[1] = best;
    o3[2] = second;
  }
}

}  // namespace rtgs

extern "C" int rtgs_keypoint_detect(const float* color_chw, const float* depth, int32_t H, int32_t W, int32_t cell, int32_t threshold,
                                    uint8_t* g8, int32_t* box5, int32_t* slots, void* stream) {
  if (!color_chw || !depth || !g8 || !box5 || !slots) return -1;
  if (H < 1 || W < 1 || (int64_t)H * W >= 2147483648LL) return -1;
  if (cell < RTGS_KEYPOINT_MIN_CELL || cell > RTGS_KEYPOINT_MAX_CELL || threshold < 0 || threshold > 255) return -1;
  const int ncx = (W + cell - 1) / cell, ncy = (H + cell - 1) / cell;
  if (ncy > 65535) return -1;
  const dim3 grid((unsigned)ncx, (unsigned)ncy), block(rtgs::KP_THREADS);
  hipLaunchKernelGGL(rtgs::keypoint_detect_kernel, grid, block, 0, (hipStream_t)stream, color_chw, depth, (int)H, (int)W, (int)cell, ncx,
                     (int)threshold, g8, box5, slots);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int rtgs_keypoint_describe(const uint8_t* g8, const int32_t* box5, int32_t H, int32_t W, int32_t n_slots, int32_t oriented,
                                      const int32_t* dirs, const uint32_t* tables, int32_t* slots, uint32_t* desc, void* stream) {
  if (!g8 || !box5 || !dirs || !tables || !slots || !desc) return -1;
  if (H < 1 || W < 1 || (int64_t)H * W >= 2147483648LL || n_slots < 0) return -1;
  if (n_slots == 0) return 0;
  const dim3 grid((unsigned)((n_slots + rtgs::KP_WAVES - 1) / rtgs::KP_WAVES)), block(rtgs::KP_THREADS);
  hipLaunchKernelGGL(rtgs::keypoint_describe_kernel, grid, block, 0, (hipStream_t)stream, g8, box5, (int)H, (int)W, (int)n_slots,
                     (int)(oriented != 0), dirs, tables, slots, desc);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int rtgs_keypoint_match(const uint32_t* desc, int64_t n_desc, const int32_t* pairs, int32_t n_pairs, int32_t max_queries,
                                   int32_t* out, int64_t n_out, void* stream) {
  if (n_pairs < 0 || n_desc < 0 || n_out < 0 || max_queries < 0 || n_pairs > 65535) return -1;
  if (n_desc >= 2147483648LL || n_out >= 2147483648LL) return -1;
  if (n_pairs == 0 || max_queries == 0) return 0;
  if (!desc || !pairs || !out || ((uintptr_t)desc & 15u)) return -1;
  const dim3 grid((unsigned)((max_queries + rtgs::KP_WAVES - 1) / rtgs::KP_WAVES), (unsigned)n_pairs), block(rtgs::KP_THREADS);
  hipLaunchKernelGGL(rtgs::keypoint_match_kernel, grid, block, 0, (hipStream_t)stream, desc, (long long)n_desc, pairs, (long long)n_out,
                     out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
