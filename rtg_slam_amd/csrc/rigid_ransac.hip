// rtgs_rigid_ransac (include/rtgs_slam.h): the match filter and the 3-D - 3-D rigid RANSAC of a batch of keyframe pairs in one
// launch.  tests/rigid_ransac_reference.py is the definition: + - * / and sqrt of float64 in a stated order, every sum over
// matches in THE WAVE ORDER of tests/place_reference.py, so the kernel matches it bit for bit.  Compiled with -ffp-contract=off.
//
// One block of 256 threads per pair.
//   filter:     256 rows of the b-against-a table a round; a ballot and the four waves' counts give every survivor its place in
//               order of i.  Its two points go to LDS (2 x 1024 x 3 float64 = 48 KiB), its (i, j) straight to `out`.
//   hypotheses: one lane per hypothesis, h = tid, tid + 256, ..  A lane fits its triplet (a sum of three in the wave order is
//               ((0 + v0) + (0 + v2)) + (0 + v1)), then walks all n matches from LDS - every lane reads the same address, a
//               broadcast - and counts.  The block reduces count << 16 | 0xFFFF - h by shuffles and four LDS words.
//   refits:     wave 0.  Lane l owns matches l, l + 64, .. (at most 16: its inlier flags are one register), which is the wave
//               order's own split, so the sums are a strided loop and six butterfly steps; the closed form then runs in every lane.
// The Jacobi sweeps are unrolled over the compile-time (p, q), so the 4 x 4 matrices stay in registers.  Vector stores only, no
// atomics, no host read; nothing depends on the order in which blocks or waves run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rtgs_slam.h"

namespace rtgs {

constexpr int RR_WAVE = 64;
constexpr int RR_WAVES = 4;
constexpr int RR_THREADS = RR_WAVE * RR_WAVES;
constexpr int RR_CAP = RTGS_RANSAC_MAX_MATCHES;
constexpr int RR_HEAD = RTGS_RANSAC_HEAD;
constexpr int RR_SWEEPS = 8;

struct RrPose {
  double R[3][3];
  double t[3];
};

__device__ __forceinline__ uint32_t rr_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

template <int P, int Q>
__device__ __forceinline__ void rr_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  if (apq != 0.0) {
    const double app = a[P][P], aqq = a[Q][Q];
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    a[P][P] = app - t * apq;
    a[Q][Q] = aqq + t * apq;
    a[P][Q] = 0.0;
    a[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r != P && r != Q) {
        const double arp = a[r][P], arq = a[r][Q];
        const double np_ = c * arp - s * arq, nq = s * arp + c * arq;
        a[r][P] = np_;
        a[P][r] = np_;
        a[r][Q] = nq;
        a[Q][r] = nq;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double vrp = v[r][P], vrq = v[r][Q];
      v[r][P] = c * vrp - s * vrq;
      v[r][Q] = s * vrp + c * vrq;
    }
  }
}

// Horn's closed form from the centroids and the nine sums S[r][c] = sum (B[r] - cb[r]) (A[c] - ca[c])
__device__ __forceinline__ void rr_pose_from_sums(const double (&ca)[3], const double (&cb)[3], const double (&S)[3][3], RrPose& out) {
  double a[4][4], v[4][4];
  a[0][0] = (S[0][0] + S[1][1]) + S[2][2];
  a[1][1] = (S[0][0] - S[1][1]) - S[2][2];
  a[2][2] = (S[1][1] - S[0][0]) - S[2][2];
  a[3][3] = (S[2][2] - S[0][0]) - S[1][1];
  a[0][1] = a[1][0] = S[1][2] - S[2][1];
  a[0][2] = a[2][0] = S[2][0] - S[0][2];
  a[0][3] = a[3][0] = S[0][1] - S[1][0];
  a[1][2] = a[2][1] = S[0][1] + S[1][0];
  a[1][3] = a[3][1] = S[2][0] + S[0][2];
  a[2][3] = a[3][2] = S[1][2] + S[2][1];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < RR_SWEEPS; ++sweep) {
    rr_rotate<0, 1>(a, v);
    rr_rotate<0, 2>(a, v);
    rr_rotate<0, 3>(a, v);
    rr_rotate<1, 2>(a, v);
    rr_rotate<1, 3>(a, v);
    rr_rotate<2, 3>(a, v);
  }
  double best = a[0][0], w = v[0][0], x = v[1][0], y = v[2][0], z = v[3][0];
#pragma unroll
  for (int m = 1; m < 4; ++m) {
    if (a[m][m] > best) {
      best = a[m][m];
      w = v[0][m];
      x = v[1][m];
      y = v[2][m];
      z = v[3][m];
    }
  }
  const double norm = sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / norm;
  x = x / norm;
  y = y / norm;
  z = z / norm;
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  out.R[0][0] = 1.0 - 2.0 * (yy + zz);
  out.R[0][1] = 2.0 * (xy - wz);
  out.R[0][2] = 2.0 * (xz + wy);
  out.R[1][0] = 2.0 * (xy + wz);
  out.R[1][1] = 1.0 - 2.0 * (xx + zz);
  out.R[1][2] = 2.0 * (yz - wx);
  out.R[2][0] = 2.0 * (xz - wy);
  out.R[2][1] = 2.0 * (yz + wx);
  out.R[2][2] = 1.0 - 2.0 * (xx + yy);
#pragma unroll
  for (int r = 0; r < 3; ++r) out.t[r] = ca[r] - ((out.R[r][0] * cb[0] + out.R[r][1] * cb[1]) + out.R[r][2] * cb[2]);
}

__device__ __forceinline__ double rr_sum3(double v0, double v1, double v2) { return ((0.0 + v0) + (0.0 + v2)) + (0.0 + v1); }

__device__ __forceinline__ double rr_wave_sum(double v) {
  for (int o = RR_WAVE / 2; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, RR_WAVE);
  return v;
}

__device__ __forceinline__ bool rr_spread(const double* __restrict__ p0, const double* __restrict__ p1, const double* __restrict__ p2) {
  const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
  const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
  const double s1 = (e1x * e1x + e1y * e1y) + e1z * e1z, s2 = (e2x * e2x + e2y * e2y) + e2z * e2z;
  const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
  return s1 > 1e-18 && s2 > 1e-18 && (cx * cx + cy * cy) + cz * cz >= 0.01 * (s1 * s2);
}

// the pose of hypothesis h; false when the triplet is skipped.  pa, pb: the n matches' points in LDS, n >= 3
__device__ __forceinline__ bool rr_hypothesis(const double* __restrict__ pa, const double* __restrict__ pb, uint32_t n, uint32_t seed, int h,
                                              RrPose& pose) {
  const uint32_t i0 = rr_mix32(seed + 3u * (uint32_t)h) % n, i1 = rr_mix32(seed + 3u * (uint32_t)h + 1u) % n,
                 i2 = rr_mix32(seed + 3u * (uint32_t)h + 2u) % n;
  if (i0 == i1 || i0 == i2 || i1 == i2) return false;
  const double *a0 = pa + 3 * i0, *a1 = pa + 3 * i1, *a2 = pa + 3 * i2, *b0 = pb + 3 * i0, *b1 = pb + 3 * i1, *b2 = pb + 3 * i2;
  if (!rr_spread(a0, a1, a2) || !rr_spread(b0, b1, b2)) return false;
  double ca[3], cb[3], S[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    ca[c] = rr_sum3(a0[c], a1[c], a2[c]) / 3.0;
    cb[c] = rr_sum3(b0[c], b1[c], b2[c]) / 3.0;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      S[r][c] = rr_sum3((b0[r] - cb[r]) * (a0[c] - ca[c]), (b1[r] - cb[r]) * (a1[c] - ca[c]), (b2[r] - cb[r]) * (a2[c] - ca[c]));
  rr_pose_from_sums(ca, cb, S, pose);
  return true;
}

__device__ __forceinline__ double rr_residual2(const RrPose& p, const double* __restrict__ a, const double* __restrict__ b) {
  const double bx = b[0], by = b[1], bz = b[2];
  const double dx = (((p.R[0][0] * bx + p.R[0][1] * by) + p.R[0][2] * bz) + p.t[0]) - a[0];
  const double dy = (((p.R[1][0] * bx + p.R[1][1] * by) + p.R[1][2] * bz) + p.t[1]) - a[1];
  const double dz = (((p.R[2][0] * bx + p.R[2][1] * by) + p.R[2][2] * bz) + p.t[2]) - a[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// wave 0: lane l's flags of matches l, l + 64, .. under `pose`, bit k for match l + 64 k; -> the wave's count in every lane
__device__ __forceinline__ int rr_wave_mask(const RrPose& pose, const double* __restrict__ pa, const double* __restrict__ pb, int n, int lane, double lim,
                                            uint32_t& mask) {
  mask = 0u;
  int k = 0;
  for (int i = lane; i < n; i += RR_WAVE, ++k)
    if (rr_residual2(pose, pa + 3 * i, pb + 3 * i) <= lim) mask |= 1u << k;
  int cnt = __popc(mask);
  for (int o = RR_WAVE / 2; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, RR_WAVE);
  return cnt;
}

// wave 0: FIT of all n matches gated by the lanes' flags, cnt of them
__device__ __forceinline__ void rr_wave_fit(const double* __restrict__ pa, const double* __restrict__ pb, int n, int lane, uint32_t mask, int cnt,
                                            RrPose& pose) {
  double sa[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0};
  int k = 0;
  for (int i = lane; i < n; i += RR_WAVE, ++k) {
    const bool in = (mask >> k) & 1u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sa[c] = sa[c] + (in ? pa[3 * i + c] : 0.0);
      sb[c] = sb[c] + (in ? pb[3 * i + c] : 0.0);
    }
  }
  double ca[3], cb[3], S[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    ca[c] = rr_wave_sum(sa[c]) / (double)cnt;
    cb[c] = rr_wave_sum(sb[c]) / (double)cnt;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) S[r][c] = 0.0;
  k = 0;
  for (int i = lane; i < n; i += RR_WAVE, ++k) {
    const bool in = (mask >> k) & 1u;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) S[r][c] = S[r][c] + (in ? (pb[3 * i + r] - cb[r]) * (pa[3 * i + c] - ca[c]) : 0.0);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) S[r][c] = rr_wave_sum(S[r][c]);
  rr_pose_from_sums(ca, cb, S, pose);
}

__global__ void __launch_bounds__(RR_THREADS) rigid_ransac_kernel(const int32_t* __restrict__ matches, long long n_matches, const double* __restrict__ xyz,
                                                                   long long n_xyz, const int32_t* __restrict__ pairs, int max_hamming, double ratio,
                                                                   int iters, double inlier_dist, uint32_t seed, int cap, long long stride,
                                                                   int32_t* __restrict__ out) {
  __shared__ double pa[3 * RR_CAP];
  __shared__ double pb[3 * RR_CAP];
  __shared__ int wave_cnt[RR_WAVES];
  __shared__ unsigned wave_key[RR_WAVES];
  const int tid = threadIdx.x, lane = tid & (RR_WAVE - 1), wave = tid >> 6;
  const int32_t* p = pairs + 6 * (long long)blockIdx.x;
  const long long mb = p[0], nb = p[1], ma = p[2], na = p[3], xa = p[4], xb = p[5];
  // block-uniform exit, before any barrier: a table that points outside the buffers is not followed
  if (mb < 0 || nb < 0 || ma < 0 || na < 0 || xa < 0 || xb < 0 || mb + nb > n_matches || ma + na > n_matches || xa + na > n_xyz ||
      xb + nb > n_xyz)
    return;
  int32_t* head = out + (long long)blockIdx.x * stride;
  int32_t* rows = head + RR_HEAD;

  // ---- filter: the survivors in order of i ----
  int base = 0;
  for (long long i0 = 0; i0 < nb; i0 += RR_THREADS) {
    const long long i = i0 + tid;
    bool keep = false;
    int j = -1;
    if (i < nb) {
      const int32_t* m = matches + 3 * (mb + i);
      j = m[0];
      const int d = m[1], second = m[2];
      keep = j >= 0 && j < na && (long long)matches[3 * (ma + j)] == i && d <= max_hamming && (double)d <= ratio * (double)second;
    }
    const unsigned long long vote = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(vote);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RR_WAVES; ++w) {
      const int c = wave_cnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    const int pos = base + before + __popcll(vote & ((1ull << lane) - 1ull));
    if (keep && pos < cap) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pa[3 * pos + c] = xyz[3 * (xa + j) + c];
        pb[3 * pos + c] = xyz[3 * (xb + i) + c];
      }
      rows[3 * pos] = (int32_t)i;
      rows[3 * pos + 1] = j;
    }
    base += total;
    __syncthreads();                                               // wave_cnt is written again in the next round
  }
  const int n = base < cap ? base : cap;
  for (int k = n + tid; k < cap; k += RR_THREADS) {
    rows[3 * k] = -1;
    rows[3 * k + 1] = -1;
    rows[3 * k + 2] = 0;
  }
  __syncthreads();                                                 // the points are in LDS (also for nb == 0: no round ran)

  // ---- hypotheses ----
  const double lim = inlier_dist * inlier_dist;
  unsigned key = 0u;
  if (n >= 3) {
    for (int h = tid; h < iters; h += RR_THREADS) {
      RrPose pose;
      if (!rr_hypothesis(pa, pb, (uint32_t)n, seed, h, pose)) continue;
      int cnt = 0;
      for (int i = 0; i < n; ++i) cnt += rr_residual2(pose, pa + 3 * i, pb + 3 * i) <= lim ? 1 : 0;
      const unsigned k = ((unsigned)cnt << 16) | (unsigned)(0xFFFF - h);
      key = k > key ? k : key;
    }
  }
  for (int o = RR_WAVE / 2; o >= 1; o >>= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)key, o, RR_WAVE);
    key = other > key ? other : key;
  }
  if (lane == 0) wave_key[wave] = key;
  __syncthreads();
  if (wave != 0) return;                                           // no barrier below
#pragma unroll
  for (int w = 1; w < RR_WAVES; ++w) key = wave_key[w] > key ? wave_key[w] : key;

  // ---- wave 0: the winner again, the refits, the outputs ----
  RrPose pose;
  uint32_t mask = 0u;
  int cnt = 0, h_best = -1;
  double rms = 0.0;
  if (key != 0u) {
    h_best = 0xFFFF - (int)(key & 0xFFFFu);
    rr_hypothesis(pa, pb, (uint32_t)n, seed, h_best, pose);
    cnt = rr_wave_mask(pose, pa, pb, n, lane, lim, mask);
    for (int round = 0; round < 3; ++round) {                      // every condition below is wave-uniform
      if (cnt < 3) break;
      RrPose p2;
      uint32_t m2;
      rr_wave_fit(pa, pb, n, lane, mask, cnt, p2);
      const int c2 = rr_wave_mask(p2, pa, pb, n, lane, lim, m2);
      if (c2 < cnt) break;
      const bool same = __all(m2 == mask);
      pose = p2;
      mask = m2;
      cnt = c2;
      if (same) break;
    }
    if (cnt > 0) {
      double acc = 0.0;
      int k = 0;
      for (int i = lane; i < n; i += RR_WAVE, ++k) {
        const double d2 = rr_residual2(pose, pa + 3 * i, pb + 3 * i);
        acc = acc + (((mask >> k) & 1u) ? d2 : 0.0);
      }
      rms = sqrt(rr_wave_sum(acc) / (double)cnt);
    }
  }
  {
    int k = 0;
    for (int i = lane; i < n; i += RR_WAVE, ++k) rows[3 * i + 2] = (int32_t)((mask >> k) & 1u);
  }
  if (lane == 0) {
    double* hd = reinterpret_cast<double*>(head);
    const bool some = key != 0u;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) hd[4 * r + c] = some ? pose.R[r][c] : 0.0;
      hd[4 * r + 3] = some ? pose.t[r] : 0.0;
    }
    hd[12] = 0.0;
    hd[13] = 0.0;
    hd[14] = 0.0;
    hd[15] = some ? 1.0 : 0.0;
    hd[16] = rms;
    head[34] = n;
    head[35] = cnt;
    head[36] = h_best;
    head[37] = base;
    head[38] = 0;
    head[39] = 0;
  }
}

}  // namespace rtgs

extern "C" int rtgs_rigid_ransac(const int32_t* matches, int64_t n_matches, const double* xyz, int64_t n_xyz, const int32_t* pairs,
                                 int32_t n_pairs, int32_t max_hamming, double ratio, int32_t iters, double inlier_dist, uint32_t seed,
                                 int32_t max_matches, int32_t* out, void* stream) {
  if (n_pairs < 0 || n_pairs > 65535 || n_matches < 0 || n_xyz < 0 || n_matches >= 2147483648LL || n_xyz >= 2147483648LL) return -1;
  if (iters < 1 || iters > RTGS_RANSAC_MAX_ITERS || max_matches < 0 || max_matches > RTGS_RANSAC_MAX_MATCHES || (max_matches & 1) || !(inlier_dist >= 0.0) || !(ratio >= 0.0)) return -1;
  if (!pairs || !out || ((uintptr_t)out & 7u) || (n_matches > 0 && !matches) || (n_xyz > 0 && (!xyz || ((uintptr_t)xyz & 7u)))) return -1;
  if (n_pairs == 0) return 0;
  const dim3 grid((unsigned)n_pairs), block(rtgs::RR_THREADS);
  hipLaunchKernelGGL(rtgs::rigid_ransac_kernel, grid, block, 0, (hipStream_t)stream, matches, (long long)n_matches, xyz, (long long)n_xyz, pairs,
                     (int)max_hamming, ratio, (int)iters, inlier_dist, seed, (int)max_matches, (long long)rtgs::RR_HEAD + 3LL * max_matches, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
