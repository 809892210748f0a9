// In-LDS sorts of ONE tile's bucket of 8-byte keys (depth bits << 32 | Gaussian id), as device functions: called by the
// sort kernels of raster_bin.hip (one workgroup per tile and size class) and by the sorting prologue of blend_fwd
// (raster_fwd.hip), which sorts its tile's list in the LDS it stages records into afterwards.  Keys are unique, so the
// order is total: whoever sorts a bucket, with however many threads, leaves the same list.
// Every thread of the workgroup calls (n is workgroup-uniform); both functions return behind a barrier, after which no
// thread touches anything but the sorted keys.
#pragma once
#include "raster_common.h"

namespace rtgs {

// Bitonic network over n2 <= THREADS keys (a power of two), ONE KEY PER THREAD in a register: thread t passes the key of
// position t (~0 beyond the list) and receives the key of position t of the sorted list.  The compare-exchanges whose
// partner sits in the same wave (j < 64: all but three of the 36 stages of 256 keys) are lane exchanges - no LDS
// traffic, no barrier; only j >= 64 goes through s_x (THREADS keys).  Blocks of n2 threads sort independently; the
// list is block 0's.  Returns behind its last barrier: nobody touches s_x any more.
// Only the blend's prologue calls this form; the sort launches keep the LDS form below for every length.
template <int THREADS>
__device__ __forceinline__ unsigned long long tile_sort_bitonic_reg(unsigned long long* s_x, unsigned long long key, int n2) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= n2; k <<= 1) {
    const bool up = (tid & k) == 0;
    for (int j = k >> 1; j > 0; j >>= 1) {
      unsigned long long other;
      if (j >= 64) {
        s_x[tid] = key;
        __syncthreads();
        other = s_x[tid ^ j];
        __syncthreads();
      } else {
        other = __shfl_xor(key, j);
      }
      // the network of tile_sort_bitonic: of the pair (a, a | j) position a keeps the smaller key where (a & k) == 0
      const bool take_min = ((tid & j) == 0) == up;
      key = (take_min == (other < key)) ? other : key;
    }
  }
  return key;
}

// Bitonic network over the next power of two >= n (n >= 2), in LDS: s_key holds that many keys, the first n sorted on
// return.  What the sort launches run, whatever the list length.
template <int THREADS>
__device__ __forceinline__ void tile_sort_bitonic(unsigned long long* s_key, const unsigned long long* __restrict__ src,
                                                  int n) {
  const int tid = threadIdx.x;
  int n2 = 2;
  while (n2 < n) n2 <<= 1;
  for (int i = tid; i < n2; i += THREADS) s_key[i] = (i < n) ? src[i] : ~0ull;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (n2 >> 1); i += THREADS) {
        const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1));     // index with bit j clear
        const int b = a | j;
        const unsigned long long ka = s_key[a], kb = s_key[b];
        const bool up = (a & k) == 0;
        if ((ka > kb) == up) { s_key[a] = kb; s_key[b] = ka; }
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------
// LDS radix sort of one tile bucket: LSD over the bytes of the depth bits that actually vary inside
// the tile (usually 3 of 4), stable within a pass (wave-ordered segments, ballot ranks), then a
// parallel fix-up that orders runs of bit-equal depths by Gaussian id.  ~6 LDS operations per key and pass instead of the
// ~1.5 x 78 stages of the bitonic network.
// kA, kB: n keys each; s_cnt: [THREADS / 64][256]; s_tot: [256]; s_or: one word.  Returns kA or kB: where the sorted keys are.
// ---------------------------------------------------------------------------------------------
template <int THREADS>
__device__ __forceinline__ unsigned long long* tile_sort_radix(unsigned long long* kA, unsigned long long* kB,
                                                               uint32_t* s_cnt, uint32_t* s_tot, uint32_t* s_or,
                                                               const unsigned long long* __restrict__ src, int n) {
  constexpr int NW = THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) *s_or = 0;
  __syncthreads();
  const uint32_t z0 = (uint32_t)(src[0] >> 32);
  uint32_t vary = 0;
  for (int i = tid; i < n; i += THREADS) {
    const unsigned long long k = src[i];
    kA[i] = k;
    vary |= (uint32_t)(k >> 32) ^ z0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) vary |= (uint32_t)__shfl_xor((int)vary, off);
  if (lane == 0 && vary) atomicOr(s_or, vary);
  __syncthreads();
  const uint32_t vbits = *s_or;
  const int seg = ((n + NW - 1) / NW + 63) & ~63;        // keys per wave, multiple of 64
  const int wlo = min(n, w * seg), whi = min(n, wlo + seg);
  for (int pass = 0; pass < 4; ++pass) {
    if (((vbits >> (8 * pass)) & 0xffu) == 0) continue;   // this byte is constant inside the tile
    const int shift = 32 + 8 * pass;
    for (int i = tid; i < NW * 256; i += THREADS) s_cnt[i] = 0;
    __syncthreads();
    for (int i = wlo + lane; i < whi; i += 64) atomicAdd(&s_cnt[w * 256 + (int)((kA[i] >> shift) & 0xff)], 1u);
    __syncthreads();
    if (tid < 256) {                                      // per digit: exclusive prefix over waves + digit total
      uint32_t run = 0;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) { const uint32_t c = s_cnt[ww * 256 + tid]; s_cnt[ww * 256 + tid] = run; run += c; }
      s_tot[tid] = run;
    }
    __syncthreads();
    if (tid < 64) {                                       // exclusive scan of the 256 digit totals by one wave
      uint32_t v0 = s_tot[4 * tid], v1 = s_tot[4 * tid + 1], v2 = s_tot[4 * tid + 2], v3 = s_tot[4 * tid + 3];
      const uint32_t mine = v0 + v1 + v2 + v3;
      uint32_t inc = mine;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, off);
        if (tid >= off) inc += o;
      }
      const uint32_t ex = inc - mine;
      s_tot[4 * tid] = ex; s_tot[4 * tid + 1] = ex + v0; s_tot[4 * tid + 2] = ex + v0 + v1; s_tot[4 * tid + 3] = ex + v0 + v1 + v2;
    }
    __syncthreads();
    for (int i0 = wlo; i0 < whi; i0 += 64) {
      const int i = i0 + lane;
      const bool act = i < whi;
      const unsigned long long k = act ? kA[i] : 0ull;
      const int d = (int)((k >> shift) & 0xff);
      unsigned long long same = __builtin_amdgcn_ballot_w64(act);
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64((d >> bit) & 1);
        same &= ((d >> bit) & 1) ? m : ~m;
      }
      if (act) {
        const unsigned long long below = same & ((1ull << lane) - 1ull);
        const uint32_t base = s_cnt[w * 256 + d] + s_tot[d];
        kB[base + (uint32_t)__popcll(below)] = k;
        if ((same >> lane) == 1ull) s_cnt[w * 256 + d] += (uint32_t)__popcll(same);   // highest lane of the group
      }
    }
    __syncthreads();
    unsigned long long* tmp = kA; kA = kB; kB = tmp;
  }
  // Runs of bit-equal depth (the bucket was filled by atomics, so equal depths arrive in arbitrary order): order them
  // by Gaussian id.  Usually there is none.  Otherwise every key finds its run with two binary searches over the
  // depth-sorted array and its rank inside the run by counting the smaller ids (broadcast LDS reads) - O(run) per key
  // and fully parallel, whatever the run length (a wall seen head-on puts hundreds of bit-equal depths into one tile).
  bool tie = false;
  for (int i = tid + 1; i < n; i += THREADS) tie |= (uint32_t)(kA[i] >> 32) == (uint32_t)(kA[i - 1] >> 32);
  if (__syncthreads_or(tie)) {
    for (int i = tid; i < n; i += THREADS) {
      const unsigned long long key = kA[i];
      const uint32_t z = (uint32_t)(key >> 32);
      int lo = 0, hi = i;                       // first index with depth == z
      while (lo < hi) { const int mid = (lo + hi) >> 1; if ((uint32_t)(kA[mid] >> 32) < z) lo = mid + 1; else hi = mid; }
      const int first = lo;
      lo = i; hi = n;                           // one past the last index with depth == z
      while (lo < hi) { const int mid = (lo + hi) >> 1; if ((uint32_t)(kA[mid] >> 32) <= z) lo = mid + 1; else hi = mid; }
      int rank = first;
      if (lo - first > 1)
        for (int j = first; j < lo; ++j) rank += (kA[j] < key) ? 1 : 0;
      else
        rank = i;
      kB[rank] = key;
    }
    __syncthreads();
    unsigned long long* tmp = kA; kA = kB; kB = tmp;
  }
  return kA;
}

}  // namespace rtgs
