// gfx950 kernels + C ABI of the RGB-D refinement with exposure compensation (include/rtgs_icp.h, "RGB-D refinement"): the normal
// equations of csrc/rgbd_align.hip with a gain and an offset of the source intensity as unknowns 7 and 8 - 36 + 8 + 4 float64
// sums - and the intensity pyramid of a composite target (the map's rendered colour, the frame's own where the model depth was
// filled from the frame).  csrc/rgbd_align.hip is unchanged: the six-unknown accumulation keeps its kernel.
// tests/rgbd_exposure_reference.py is the definition, matched bit for bit; built with -ffp-contract=off (Makefile
// EXTRA_rgbd_exposure): every float32 and float64 step below is one correctly rounded operation.
//
// The pixel is rgbd_align.hip's with one change: the source intensity goes through Ic = alpha I_src, Ic = Ic + beta (two rounded
// float32 steps) before r_I = value - Ic, and the Huber weight is taken on that r_I.  J8 = (J_I[0..5], -I_src, -1) with the raw
// I_src.  H[k] = (geo and i, j < 6 ? J_G[i] J_G[j] : +0) + (c J8[i]) J8[j] for i <= j < 8 row-major (36), b[i] likewise (8), then
// sum r_G^2, the geometric count, sum w r_I^2, the photometric count.
//
// Two launches per evaluation on the caller's stream, as csrc/rgbd_align.hip:
// chunks     one workgroup of 256 threads (4 waves of 64) per chunk of 1024 pixels.  Thread s is slot s: it adds the terms of the
//            pixels 1024 chunk + s + 256 k, k = 0..3, to 48 float64 registers that start at +0 (a sum that starts at +0 is never
//            -0, so a pixel whose photometric gate fails may be skipped, and the 15 + 2 entries of rows / columns 6 and 7, which
//            have no geometric part, add their photometric product alone: the +0 in front of it would change no bit).  Then the
//            tree: six __shfl_down steps inside each wave, the four wave values through LDS, (w0 + w1) + (w2 + w3) by the first
//            48 threads, which store the chunk's 48 values to the scratch.
// total      one workgroup: slot s adds the chunk values s, s + 256, ... in order, the same tree, sums_out[48].
// No atomics, no host read.  A pointer is dereferenced only after its gate: the source vertex always, the target vertex once the
// pixel projects into the view with positive depths, everything else (source normal and intensity, target normal, the four target
// intensities) once the photometric gate has passed.  Index range: 0 < u < W-1 and 0 < v < H-1 hold before any float becomes an
// integer, so the nearest pixel lies in [0, W-1] x [0, H-1] and the bilinear corners in [0, W-2] + {0, 1} x [0, H-2] + {0, 1}.
// Registers: 48 float64 accumulators are 96 VGPRs; the figures the compiler reports are in DESIGN.md 5b (no scratch).
#include "../../include/rtgs_icp.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace rtgs_rgbd_exposure_k {

constexpr int NT = 256;
constexpr int WAVE = 64;
constexpr int WAVES = NT / WAVE;
constexpr int CHUNK = 1024;
constexpr int OUT = RTGS_RGBD_EXPOSURE_OUT;
constexpr int NU = 8;                        // unknowns: rotation, translation, gain, offset
constexpr int NH = NU * (NU + 1) / 2;        // 36
static_assert(CHUNK % NT == 0 && WAVES == 4 && OUT <= NT && OUT == NH + NU + 4, "the tree below is written for 4 waves of 64");

// ---- the composite target and its pyramid ----

// replaced = the model depth was filled from the frame here: the frame's grey taken into the map's exposure; else the render's
__global__ void __launch_bounds__(NT) composite_kernel(const float* __restrict__ render, const float* __restrict__ frame,
                                                       const float* __restrict__ depth_rendered,
                                                       const float* __restrict__ depth_filled, float alpha, float beta, int64_t n,
                                                       float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  if (depth_filled[i] != depth_rendered[i]) {
    const float g = (0.299f * frame[i] + 0.587f * frame[n + i]) + 0.114f * frame[2 * n + i];
    const float a = alpha * g;
    out[i] = a + beta;
  } else {
    out[i] = (0.299f * render[i] + 0.587f * render[n + i]) + 0.114f * render[2 * n + i];
  }
}

// fine [Hf, Wf] -> coarse [Hf >> 1, Wf >> 1]; the rows and columns an odd size leaves over are dropped
__global__ void __launch_bounds__(NT) half_kernel(const float* __restrict__ fine, int Wf, int h, int w, float* __restrict__ coarse) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= (int64_t)h * w) return;
  const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
  const float* r0 = fine + (int64_t)(2 * y) * Wf + 2 * x;
  const float* r1 = r0 + Wf;
  coarse[i] = ((r0[0] + r0[1]) + (r1[0] + r1[1])) * 0.25f;
}

// ---- accumulation ----

struct Geom {
  float fx, fy, cx, cy, Wm1, Hm1, hw, hh, dist_thr, cos_thr, huber, alpha, beta;
  double lam2;
  int W;
};

// 256 slots -> one value per k, written to dst[k] by thread k.  Every thread of the workgroup calls it.
__device__ __forceinline__ void tree(double (&acc)[OUT], double* __restrict__ lds, double* __restrict__ dst) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < OUT; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = WAVE / 2; o >= 1; o >>= 1) v = v + __shfl_down(v, o, WAVE);      // lane 0 only ever reads lanes l + o < 2 o
    if (lane == 0) lds[wave * OUT + k] = v;
  }
  __syncthreads();
  if (threadIdx.x < OUT) {
    const int k = threadIdx.x;
    dst[k] = (lds[k] + lds[OUT + k]) + (lds[2 * OUT + k] + lds[3 * OUT + k]);
  }
}

__global__ void __launch_bounds__(NT) chunks_kernel(const float* __restrict__ vs, const float* __restrict__ ns,
                                                    const float* __restrict__ is, const float* __restrict__ vt,
                                                    const float* __restrict__ nt, const float* __restrict__ it, int64_t n,
                                                    const float* __restrict__ K, const float* __restrict__ pose, Geom g,
                                                    double* __restrict__ partial) {
  __shared__ double lds[WAVES * OUT];
  double acc[OUT];
#pragma unroll
  for (int k = 0; k < OUT; ++k) acc[k] = 0.0;
  const float R00 = pose[0], R01 = pose[1], R02 = pose[2], t0 = pose[3];
  const float R10 = pose[4], R11 = pose[5], R12 = pose[6], t1 = pose[7];
  const float R20 = pose[8], R21 = pose[9], R22 = pose[10], t2 = pose[11];
  g.fx = K[0]; g.fy = K[4]; g.cx = K[2]; g.cy = K[5];
  const int64_t base = (int64_t)blockIdx.x * CHUNK + threadIdx.x;
#pragma unroll 1
  for (int step = 0; step < CHUNK / NT; ++step) {
    const int64_t i = base + (int64_t)step * NT;
    if (i >= n) break;
    const float px = vs[i * 3], py = vs[i * 3 + 1], pz = vs[i * 3 + 2];
    const float qx = ((R00 * px + R01 * py) + R02 * pz) + t0;
    const float qy = ((R10 * px + R11 * py) + R12 * pz) + t1;
    const float qz = ((R20 * px + R21 * py) + R22 * pz) + t2;
    const float u = (qx / qz) * g.fx + g.cx;
    const float v = (qy / qz) * g.fy + g.cy;
    const bool inview = (u > 0.f) && (u < g.Wm1) && (v > 0.f) && (v < g.Hm1);             // a NaN fails
    if (!(inview && pz > 0.f && qz > 0.f)) continue;
    // the nearest pixel of rtgs_icp_step (grid_sample nearest, border, align_corners)
    float ix = (((u / g.hw - 1.f) + 1.f) / 2.f) * g.Wm1, iy = (((v / g.hh - 1.f) + 1.f) / 2.f) * g.Hm1;
    ix = fminf(g.Wm1, fmaxf(ix, 0.f));
    iy = fminf(g.Hm1, fmaxf(iy, 0.f));
    const int64_t j = (int64_t)nearbyintf(iy) * g.W + (int64_t)nearbyintf(ix);
    const float gx_ = vt[j * 3], gy_ = vt[j * 3 + 1], gz_ = vt[j * 3 + 2];
    if (!(gz_ > 0.f)) continue;
    const float e0 = qx - gx_, e1 = qy - gy_, e2 = qz - gz_;
    if (!(sqrtf((e0 * e0 + e1 * e1) + e2 * e2) <= g.dist_thr)) continue;
    // ---- the photometric gate has passed ----
    const float m0 = nt[j * 3], m1 = nt[j * 3 + 1], m2 = nt[j * 3 + 2];
    const float n0 = ns[i * 3], n1 = ns[i * 3 + 1], n2 = ns[i * 3 + 2];
    const float rn0 = (R00 * n0 + R01 * n1) + R02 * n2;
    const float rn1 = (R10 * n0 + R11 * n1) + R12 * n2;
    const float rn2 = (R20 * n0 + R21 * n1) + R22 * n2;
    const bool geo = ((rn0 * m0 + rn1 * m1) + rn2 * m2) > g.cos_thr;
    const float rG = (m0 * e0 + m1 * e1) + m2 * e2;
    float JG[6], J8[NU];
    JG[0] = qy * m2 - qz * m1;
    JG[1] = qz * m0 - qx * m2;
    JG[2] = qx * m1 - qy * m0;
    JG[3] = m0; JG[4] = m1; JG[5] = m2;
    const float x0f = floorf(u), y0f = floorf(v);
    const float a = u - x0f, b = v - y0f;
    const float* c0 = it + (int64_t)y0f * g.W + (int64_t)x0f;
    const float* c1 = c0 + g.W;
    const float i00 = c0[0], i10 = c0[1], i01 = c1[0], i11 = c1[1];
    const float top = (1.f - a) * i00 + a * i10;
    const float bot = (1.f - a) * i01 + a * i11;
    const float value = (1.f - b) * top + b * bot;
    const float gx = (1.f - b) * (i10 - i00) + b * (i11 - i01);
    const float gy = (1.f - a) * (i01 - i00) + a * (i11 - i10);
    const float Is = is[i];
    float Ic = g.alpha * Is;                                     // the source intensity in the target's exposure
    Ic = Ic + g.beta;
    const float rI = value - Ic;
    const float sx = gx * g.fx, sy = gy * g.fy;
    const float d0 = sx / qz, d1 = sy / qz, d2 = -((sx * qx + sy * qy) / (qz * qz));
    J8[0] = qy * d2 - qz * d1;
    J8[1] = qz * d0 - qx * d2;
    J8[2] = qx * d1 - qy * d0;
    J8[3] = d0; J8[4] = d1; J8[5] = d2;
    J8[6] = -Is; J8[7] = -1.f;
    const float ar = fabsf(rI);
    const float w = ar <= g.huber ? 1.f : g.huber / ar;
    // ---- float64 terms on the widened values ----
    const double wd = (double)w, c = wd * g.lam2, rGd = (double)rG, rId = (double)rI;
    double G[6], P[NU], cP[NU];
#pragma unroll
    for (int k = 0; k < 6; ++k) G[k] = (double)JG[k];
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      P[k] = (double)J8[k];
      cP[k] = c * P[k];
    }
    int k = 0;
#pragma unroll
    for (int r = 0; r < NU; ++r)
#pragma unroll
      for (int s = r; s < NU; ++s) {
        if (s < 6) {
          const double tg = geo ? G[r] * G[s] : 0.0;
          acc[k] = acc[k] + (tg + cP[r] * P[s]);
        } else {
          acc[k] = acc[k] + cP[r] * P[s];
        }
        ++k;
      }
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      if (r < 6) {
        const double tg = geo ? G[r] * rGd : 0.0;
        acc[NH + r] = acc[NH + r] + (tg + cP[r] * rId);
      } else {
        acc[NH + r] = acc[NH + r] + cP[r] * rId;
      }
    }
    acc[NH + NU] = acc[NH + NU] + (geo ? rGd * rGd : 0.0);
    acc[NH + NU + 1] = acc[NH + NU + 1] + (geo ? 1.0 : 0.0);
    acc[NH + NU + 2] = acc[NH + NU + 2] + wd * (rId * rId);
    acc[NH + NU + 3] = acc[NH + NU + 3] + 1.0;
  }
  tree(acc, lds, partial + (int64_t)blockIdx.x * OUT);
}

__global__ void __launch_bounds__(NT) total_kernel(const double* __restrict__ partial, int64_t chunks, double* __restrict__ out) {
  __shared__ double lds[WAVES * OUT];
  double acc[OUT];
#pragma unroll
  for (int k = 0; k < OUT; ++k) acc[k] = 0.0;
  for (int64_t ch = threadIdx.x; ch < chunks; ch += NT) {
#pragma unroll
    for (int k = 0; k < OUT; ++k) acc[k] = acc[k] + partial[ch * OUT + k];
  }
  tree(acc, lds, out);
}

}  // namespace rtgs_rgbd_exposure_k

extern "C" {

using namespace rtgs_rgbd_exposure_k;

int rtgs_rgbd_target_intensity(const float* render_color, const float* frame_color, const float* depth_rendered,
                               const float* depth_filled, float alpha, float beta, int32_t H, int32_t W, int32_t levels,
                               float* const* out_host, void* stream) {
  if (!render_color || !frame_color || !depth_rendered || !depth_filled || !out_host) return -1;
  if (H <= 0 || W <= 0 || levels <= 0 || levels > RTGS_ICP_MAX_LEVELS) return -1;
  if ((int64_t)H * W >= 0x80000000LL) return -1;
  if ((H >> (levels - 1)) <= 0 || (W >> (levels - 1)) <= 0) return -1;
  for (int l = 0; l < levels; ++l)
    if (!out_host[l]) return -1;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(composite_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, render_color, frame_color,
                     depth_rendered, depth_filled, alpha, beta, n, out_host[levels - 1]);
  for (int l = levels - 2; l >= 0; --l) {
    const int sh = levels - 1 - l;
    const int h = H >> sh, w = W >> sh, Wf = W >> (sh - 1);
    const int64_t m = (int64_t)h * w;
    hipLaunchKernelGGL(half_kernel, dim3((unsigned)((m + NT - 1) / NT)), dim3(NT), 0, s, (const float*)out_host[l + 1], Wf, h, w,
                       out_host[l]);
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

size_t rtgs_rgbd_align_exposure_scratch_bytes(int32_t H, int32_t W) {
  if (H <= 0 || W <= 0 || (int64_t)H * W >= 0x80000000LL) return 0;
  return (size_t)(((int64_t)H * W + CHUNK - 1) / CHUNK) * OUT * sizeof(double);
}

int rtgs_rgbd_align_accumulate_exposure(const float* vertex_src, const float* normal_src, const float* intensity_src,
                                        const float* vertex_tgt, const float* normal_tgt, const float* intensity_tgt, int32_t H,
                                        int32_t W, const float* K, const float* pose, float distance_threshold,
                                        float cos_threshold, float photo_weight, float huber, float alpha, float beta,
                                        double* sums_out, void* scratch, void* stream) {
  if (H <= 0 || W <= 0 || (int64_t)H * W >= 0x80000000LL) return -1;
  if (!vertex_src || !normal_src || !intensity_src || !vertex_tgt || !normal_tgt || !intensity_tgt || !K || !pose || !sums_out ||
      !scratch)
    return -1;
  if (!(huber >= 0.f) || !(photo_weight >= 0.f)) return -1;                        // negative or NaN
  if (alpha != alpha || beta != beta) return -1;                                   // NaN
  const int64_t n = (int64_t)H * W;
  const int64_t chunks = (n + CHUNK - 1) / CHUNK;                                  // < 2^21
  Geom g;
  g.fx = g.fy = g.cx = g.cy = 0.f;                                                 // read from K on the device
  g.Wm1 = (float)(W - 1); g.Hm1 = (float)(H - 1);
  g.hw = g.Wm1 / 2.f; g.hh = g.Hm1 / 2.f;
  g.dist_thr = distance_threshold; g.cos_thr = cos_threshold; g.huber = huber;
  g.alpha = alpha; g.beta = beta;
  g.lam2 = (double)photo_weight * (double)photo_weight;
  g.W = W;
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)scratch;
  hipLaunchKernelGGL(chunks_kernel, dim3((unsigned)chunks), dim3(NT), 0, s, vertex_src, normal_src, intensity_src, vertex_tgt,
                     normal_tgt, intensity_tgt, n, K, pose, g, partial);
  hipLaunchKernelGGL(total_kernel, dim3(1), dim3(NT), 0, s, (const double*)partial, chunks, sums_out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
