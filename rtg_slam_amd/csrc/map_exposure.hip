// gfx950 kernels + C ABI of the mapper's exposure stage (include/rtgs_slam.h, "map exposure"): a gain and an offset per frame that
// take the frame's colour into the map's exposure, fitted by iteratively reweighted least squares on the pixels where the frame
// and the map rendered at the frame's pose see the same surface, and the launch that writes the corrected colour.
// tests/map_exposure_reference.py is the definition, matched bit for bit; built with -ffp-contract=off (Makefile
// EXTRA_map_exposure): every float32 and float64 step below is one correctly rounded operation.
//
// Two launches per iteration on the caller's stream, no atomics, no host read:
// chunks     one workgroup of 256 threads (4 waves of 64) per chunk of 1024 pixels in row-major order.  Thread s is slot s: it adds
//            the eight float64 terms of the pixels 1024 chunk + s + 256 k, k = 0..3, to registers that start at +0 (a sum that
//            starts at +0 is never -0, so an invalid pixel may be skipped).  Then the tree of csrc/rgbd_align.hip: six
//            __shfl_down steps inside each wave, the four wave values through LDS, (w0 + w1) + (w2 + w3).
// total      one workgroup: slot s adds the chunk values s, s + 256, ... in order, the same tree; thread 0 then solves the 2 x 2
//            system in float64, accepts or rejects, and writes the state.
// Both kernels read the state's code first: from iteration 1 on a frame whose fit was rejected launches workgroups that return at
// once.  Every array is indexed by the pixel index i < H W alone; no index is computed from data.
// The state: RTGS_MAP_EXPOSURE_STATE doubles - alpha, beta, the frame's start (alpha, beta), the code, the iterations accepted for
// this frame, two spare, the eight sums of the last iteration that ran.
#include "../../include/rtgs_slam.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)                                   // the solve below is float64 step by step, as numpy's

namespace rtgs_map_exposure_k {

constexpr int NT = 256;
constexpr int WAVE = 64;
constexpr int WAVES = NT / WAVE;
constexpr int CHUNK = 1024;
constexpr int OUT = RTGS_MAP_EXPOSURE_SUMS;
constexpr int STATE = RTGS_MAP_EXPOSURE_STATE;
constexpr int S_ALPHA = 0, S_BETA = 1, S_ALPHA0 = 2, S_BETA0 = 3, S_CODE = 4, S_ITERS = 5, S_SUMS = 8;
static_assert(CHUNK % NT == 0 && WAVES == 4 && OUT == 8 && S_SUMS + OUT == STATE, "the tree below is written for 4 waves of 64");

struct Gates {
  float huber, cutoff, depth_gate, t_gate, lo, hi;
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

__global__ void __launch_bounds__(NT) chunks_kernel(const float* __restrict__ fc, const float* __restrict__ fd,
                                                    const float* __restrict__ rc, const float* __restrict__ rd,
                                                    const float* __restrict__ T, int64_t n, int iteration, Gates g,
                                                    const double* __restrict__ state, double* __restrict__ partial) {
  __shared__ double lds[WAVES * OUT];
  if (iteration > 0 && state[S_CODE] != 0.0) return;                             // the frame's fit has ended: uniform over the grid
  const float alpha = (float)state[S_ALPHA], beta = (float)state[S_BETA];
  double acc[OUT];
#pragma unroll
  for (int k = 0; k < OUT; ++k) acc[k] = 0.0;
  const int64_t base = (int64_t)blockIdx.x * CHUNK + threadIdx.x;
#pragma unroll 1
  for (int step = 0; step < CHUNK / NT; ++step) {
    const int64_t i = base + (int64_t)step * NT;
    if (i >= n) break;
    const float d = fd[i], m = rd[i];
    if (!(d > 0.f && m > 0.f && fabsf(d - m) <= g.depth_gate && T[i] <= g.t_gate)) continue;          // a NaN fails
    const float c0 = fc[i], c1 = fc[n + i], c2 = fc[2 * n + i];
    if (!(c0 >= g.lo && c0 <= g.hi && c1 >= g.lo && c1 <= g.hi && c2 >= g.lo && c2 <= g.hi)) continue;
    const float r0 = rc[i], r1 = rc[n + i], r2 = rc[2 * n + i];
    if (!(isfinite(r0) && isfinite(r1) && isfinite(r2))) continue;
    const float I = (0.299f * c0 + 0.587f * c1) + 0.114f * c2;
    const float R = (0.299f * r0 + 0.587f * r1) + 0.114f * r2;
    float Ic = alpha * I;                                        // the frame's intensity in the map's exposure
    Ic = Ic + beta;
    const float r = Ic - R;
    const float a = fabsf(r);
    float w = a <= g.huber ? 1.f : g.huber / a;
    if (iteration > 0 && a > g.cutoff) w = 0.f;
    const double wd = (double)w, Id = (double)I, Rd = (double)R, rr = (double)r;
    const double wI = wd * Id;
    acc[0] = acc[0] + wd;
    acc[1] = acc[1] + wI;
    acc[2] = acc[2] + wd * Rd;
    acc[3] = acc[3] + wI * Id;
    acc[4] = acc[4] + wI * Rd;
    acc[5] = acc[5] + wd * (rr * rr);
    acc[6] = acc[6] + 1.0;
    acc[7] = acc[7] + (a <= g.huber ? 1.0 : 0.0);
  }
  tree(acc, lds, partial + (int64_t)blockIdx.x * OUT);
}

__global__ void __launch_bounds__(NT) total_kernel(const double* __restrict__ partial, int64_t chunks, int iteration, double var_min,
                                                   double min_valid, double* __restrict__ state) {
  __shared__ double lds[WAVES * OUT];
  __shared__ double S[OUT];
  if (iteration > 0 && state[S_CODE] != 0.0) return;             // read by every thread before the barrier thread 0 writes behind
  double acc[OUT];
#pragma unroll
  for (int k = 0; k < OUT; ++k) acc[k] = 0.0;
  for (int64_t ch = threadIdx.x; ch < chunks; ch += NT) {
#pragma unroll
    for (int k = 0; k < OUT; ++k) acc[k] = acc[k] + partial[ch * OUT + k];
  }
  tree(acc, lds, S);
  __syncthreads();
  if (threadIdx.x < OUT) state[S_SUMS + threadIdx.x] = S[threadIdx.x];
  if (threadIdx.x != 0) return;
  double a0 = state[S_ALPHA0], b0 = state[S_BETA0], done = state[S_ITERS];
  if (iteration == 0) {                                           // the frame begins: what the last frame ended with
    a0 = state[S_ALPHA];
    b0 = state[S_BETA];
    done = 0.0;
  }
  double code = 0.0, alpha = a0, beta = b0;
  if (!(S[6] >= min_valid)) {
    code = 1.0;
  } else if (!(S[0] > 0.0)) {
    code = 2.0;
  } else {
    const double det = S[0] * S[3] - S[1] * S[1];
    if (!(det > var_min * (S[0] * S[0]))) {
      code = 3.0;
    } else {
      const double al = (S[0] * S[4] - S[1] * S[2]) / det;
      const double be = (S[2] - al * S[1]) / S[0];
      if (!(isfinite(al) && isfinite(be))) {
        code = 4.0;
      } else if (!(al >= 0.25 && al <= 4.0 && fabs(be) <= 0.5)) {
        code = 5.0;
      } else {
        alpha = al;
        beta = be;
        done = done + 1.0;
      }
    }
  }
  state[S_ALPHA] = alpha;
  state[S_BETA] = beta;
  state[S_ALPHA0] = a0;
  state[S_BETA0] = b0;
  state[S_CODE] = code;
  state[S_ITERS] = done;
}

// one thread per pixel: the three channels, both layouts
__global__ void __launch_bounds__(NT) apply_kernel(const float* __restrict__ color, int64_t n, const double* __restrict__ state,
                                                   float* __restrict__ out_chw, float* __restrict__ out_hwc) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const float alpha = (float)state[S_ALPHA], beta = (float)state[S_BETA];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = alpha * color[c * n + i];
    v = v + beta;
    v = fminf(fmaxf(v, 0.f), 1.f);                               // a NaN becomes 0
    out_chw[c * n + i] = v;
    out_hwc[3 * i + c] = v;
  }
}

static bool size_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && (int64_t)H * W < 0x80000000LL; }

}  // namespace rtgs_map_exposure_k

extern "C" {

using namespace rtgs_map_exposure_k;

size_t rtgs_map_exposure_scratch_bytes(int32_t H, int32_t W) {
  if (!size_ok(H, W)) return 0;
  return (size_t)(((int64_t)H * W + CHUNK - 1) / CHUNK) * OUT * sizeof(double);
}

int rtgs_map_exposure_fit(const float* frame_color_chw, const float* frame_depth, const float* render_color_chw,
                          const float* render_depth, const float* T_map, int32_t H, int32_t W, int32_t iteration, float huber,
                          float cut, float depth_gate, float t_gate, float lo, float hi, double var_min, int64_t min_valid,
                          double* state, void* scratch, void* stream) {
  if (!size_ok(H, W) || iteration < 0) return -1;
  if (!frame_color_chw || !frame_depth || !render_color_chw || !render_depth || !T_map || !state || !scratch) return -1;
  if (!(huber > 0.f) || !(cut >= 1.f) || !(depth_gate >= 0.f) || !(lo <= hi) || !(var_min >= 0.0) || min_valid < 1)   // or NaN
    return -1;
  if (t_gate != t_gate) return -1;
  const int64_t n = (int64_t)H * W;
  const int64_t chunks = (n + CHUNK - 1) / CHUNK;                                  // < 2^21
  Gates g;
  g.huber = huber;
  g.cutoff = cut * huber;                                                          // one rounded float32 product
  g.depth_gate = depth_gate; g.t_gate = t_gate; g.lo = lo; g.hi = hi;
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)scratch;
  hipLaunchKernelGGL(chunks_kernel, dim3((unsigned)chunks), dim3(NT), 0, s, frame_color_chw, frame_depth, render_color_chw,
                     render_depth, T_map, n, (int)iteration, g, (const double*)state, partial);
  hipLaunchKernelGGL(total_kernel, dim3(1), dim3(NT), 0, s, (const double*)partial, chunks, (int)iteration, var_min,
                     (double)min_valid, state);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_map_exposure_apply(const float* color_chw, int32_t H, int32_t W, const double* state, float* out_chw, float* out_hwc,
                            void* stream) {
  if (!size_ok(H, W) || !color_chw || !state || !out_chw || !out_hwc) return -1;
  if (out_chw == color_chw || out_hwc == color_chw) return -1;         // the raw colour stays what it is
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(apply_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, color_chw, n, state,
                     out_chw, out_hwc);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
