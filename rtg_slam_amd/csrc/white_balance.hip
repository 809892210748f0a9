// gfx950 kernels + C ABI of the white balance fit (include/rtgs_slam.h, "white balance"): a gain and an offset per colour channel
// from one picture to another, fitted by the iteratively reweighted least squares of csrc/map_exposure.hip on four regressions at
// once - k = 0 on the greys exactly as that file forms them, k = 1..3 on the channels themselves - and the launch that writes the
// corrected colour.  tests/white_balance_reference.py is the definition, matched bit for bit; built with -ffp-contract=off
// (Makefile EXTRA_white_balance): every float32 and float64 step below is one correctly rounded operation.
//
// Two launches per iteration on the caller's stream, no atomics, no host read; the structure is map_exposure.hip's:
// chunks     one workgroup of 256 threads (4 waves of 64) per chunk of 1024 pixels in row-major order.  Thread s is slot s: it adds
//            the 29 float64 terms of the pixels 1024 chunk + s + 256 k, k = 0..3, to registers that start at +0 (a sum that starts
//            at +0 is never -0, so an invalid pixel may be skipped).  Then six __shfl_down steps inside each wave, the four wave
//            values through LDS, (w0 + w1) + (w2 + w3).  The row of a chunk is padded to 32 doubles; the three spare stay +0.
// total      one workgroup: slot s adds the chunk values s, s + 256, ... in order, the same tree; thread 0 then solves the four
//            2 x 2 systems in float64 and applies the frame rule.
// Both kernels read the frame's code first: from iteration 1 on a frame whose fit has ended launches workgroups that return at
// once.  Every array is indexed by the pixel index i < H W alone; no index is computed from data.
#include "../../include/rtgs_slam.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)                                   // the solve below is float64 step by step, as numpy's

namespace rtgs_white_balance_k {

constexpr int NT = 256;
constexpr int WAVE = 64;
constexpr int WAVES = NT / WAVE;
constexpr int CHUNK = 1024;
constexpr int REGS = RTGS_WHITE_BALANCE_REGRESSIONS;
constexpr int PER = 7;                                           // sums per regression
constexpr int USED = REGS * PER + 1;                             // and the valid pixels
constexpr int OUT = RTGS_WHITE_BALANCE_SUMS;                     // the padded row
constexpr int VALID = RTGS_WHITE_BALANCE_VALID;
constexpr int REG = RTGS_WHITE_BALANCE_REG;
constexpr int S_FRAME = RTGS_WHITE_BALANCE_FRAME_AT, S_SUMS = RTGS_WHITE_BALANCE_SUMS_AT;
constexpr int R_ALPHA = 0, R_BETA = 1, R_ALPHA0 = 2, R_BETA0 = 3, R_CODE = 4, R_ITERS = 5;
static_assert(CHUNK % NT == 0 && WAVES == 4 && USED == 29 && VALID == REGS * PER && USED <= OUT && OUT <= WAVE,
              "the tree below is written for 4 waves of 64");
static_assert(REGS * REG == S_FRAME && S_FRAME + 8 == S_SUMS && S_SUMS + OUT == RTGS_WHITE_BALANCE_STATE, "the state's layout");

struct Gates {
  float huber, cutoff, depth_gate, t_gate, src_lo, src_hi, dst_lo, dst_hi;
};

// 256 slots -> one value per k < USED, written to dst[k] by thread k; the spare of the row are written +0.  Every thread of the
// workgroup calls it.
__device__ __forceinline__ void tree(double (&acc)[USED], double* __restrict__ lds, double* __restrict__ dst) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < USED; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = WAVE / 2; o >= 1; o >>= 1) v = v + __shfl_down(v, o, WAVE);      // lane 0 only ever reads lanes l + o < 2 o
    if (lane == 0) lds[wave * OUT + k] = v;
  }
  __syncthreads();
  if (threadIdx.x < OUT) {
    const int k = threadIdx.x;
    dst[k] = k < USED ? (lds[k] + lds[OUT + k]) + (lds[2 * OUT + k] + lds[3 * OUT + k]) : 0.0;
  }
}

// one regression's terms of one pixel: source value s, target value t
__device__ __forceinline__ void add_terms(double* __restrict__ acc, float s, float t, float alpha, float beta, int iteration,
                                          const Gates& g) {
  float sc = alpha * s;                                          // the source value in the target's exposure
  sc = sc + beta;
  const float r = sc - t;
  const float a = fabsf(r);
  float w = a <= g.huber ? 1.f : g.huber / a;
  if (iteration > 0 && a > g.cutoff) w = 0.f;
  const double wd = (double)w, sd = (double)s, td = (double)t, rr = (double)r;
  const double ws = wd * sd;
  acc[0] = acc[0] + wd;
  acc[1] = acc[1] + ws;
  acc[2] = acc[2] + wd * td;
  acc[3] = acc[3] + ws * sd;
  acc[4] = acc[4] + ws * td;
  acc[5] = acc[5] + wd * (rr * rr);
  acc[6] = acc[6] + (a <= g.huber ? 1.0 : 0.0);
}

__device__ __forceinline__ bool in_range(float c, float lo, float hi) { return c >= lo && c <= hi && isfinite(c); }   // a NaN fails

__global__ void __launch_bounds__(NT) chunks_kernel(const float* __restrict__ sc, const float* __restrict__ sd,
                                                    const float* __restrict__ tc, const float* __restrict__ td,
                                                    const float* __restrict__ T, int64_t n, int iteration, Gates g,
                                                    const double* __restrict__ state, double* __restrict__ partial) {
  __shared__ double lds[WAVES * OUT];
  if (iteration > 0 && state[S_FRAME] != 0.0) return;                            // the frame's fit has ended: uniform over the grid
  float alpha[REGS], beta[REGS];
#pragma unroll
  for (int k = 0; k < REGS; ++k) {
    alpha[k] = (float)state[k * REG + R_ALPHA];
    beta[k] = (float)state[k * REG + R_BETA];
  }
  double acc[USED];
#pragma unroll
  for (int k = 0; k < USED; ++k) acc[k] = 0.0;
  const int64_t base = (int64_t)blockIdx.x * CHUNK + threadIdx.x;
#pragma unroll 1
  for (int step = 0; step < CHUNK / NT; ++step) {
    const int64_t i = base + (int64_t)step * NT;
    if (i >= n) break;
    const float d = sd[i], m = td[i];
    if (!(d > 0.f && m > 0.f && fabsf(d - m) <= g.depth_gate && T[i] <= g.t_gate)) continue;          // a NaN fails
    const float s1 = sc[i], s2 = sc[n + i], s3 = sc[2 * n + i];
    if (!(in_range(s1, g.src_lo, g.src_hi) && in_range(s2, g.src_lo, g.src_hi) && in_range(s3, g.src_lo, g.src_hi))) continue;
    const float t1 = tc[i], t2 = tc[n + i], t3 = tc[2 * n + i];
    if (!(in_range(t1, g.dst_lo, g.dst_hi) && in_range(t2, g.dst_lo, g.dst_hi) && in_range(t3, g.dst_lo, g.dst_hi))) continue;
    const float s0 = (0.299f * s1 + 0.587f * s2) + 0.114f * s3;
    const float t0 = (0.299f * t1 + 0.587f * t2) + 0.114f * t3;
    add_terms(acc + 0 * PER, s0, t0, alpha[0], beta[0], iteration, g);
    add_terms(acc + 1 * PER, s1, t1, alpha[1], beta[1], iteration, g);
    add_terms(acc + 2 * PER, s2, t2, alpha[2], beta[2], iteration, g);
    add_terms(acc + 3 * PER, s3, t3, alpha[3], beta[3], iteration, g);
    acc[VALID] = acc[VALID] + 1.0;
  }
  tree(acc, lds, partial + (int64_t)blockIdx.x * OUT);
}

// The tests of map_exposure.hip's total_kernel on one regression's sums -> its code; (al, be) are written when it is 0.
__device__ __forceinline__ double solve(const double* __restrict__ S, double valid, double min_valid, double var_min, double& al,
                                        double& be) {
  if (!(valid >= min_valid)) return 1.0;
  if (!(S[0] > 0.0)) return 2.0;
  const double det = S[0] * S[3] - S[1] * S[1];
  if (!(det > var_min * (S[0] * S[0]))) return 3.0;
  al = (S[0] * S[4] - S[1] * S[2]) / det;
  be = (S[2] - al * S[1]) / S[0];
  if (!(isfinite(al) && isfinite(be))) return 4.0;
  if (!(al >= 0.25 && al <= 4.0 && fabs(be) <= 0.5)) return 5.0;
  return 0.0;
}

__global__ void __launch_bounds__(NT) total_kernel(const double* __restrict__ partial, int64_t chunks, int iteration, double var_min,
                                                   double min_valid, double* __restrict__ state) {
  __shared__ double lds[WAVES * OUT];
  __shared__ double S[OUT];
  if (iteration > 0 && state[S_FRAME] != 0.0) return;            // read by every thread before the barrier thread 0 writes behind
  double acc[USED];
#pragma unroll
  for (int k = 0; k < USED; ++k) acc[k] = 0.0;
  for (int64_t ch = threadIdx.x; ch < chunks; ch += NT) {
#pragma unroll
    for (int k = 0; k < USED; ++k) acc[k] = acc[k] + partial[ch * OUT + k];
  }
  tree(acc, lds, S);
  __syncthreads();
  if (threadIdx.x < OUT) state[S_SUMS + threadIdx.x] = S[threadIdx.x];
  if (threadIdx.x != 0) return;
  double a0[REGS], b0[REGS], done[REGS], code[REGS], alpha[REGS], beta[REGS];
#pragma unroll
  for (int k = 0; k < REGS; ++k) {
    const double* r = state + k * REG;
    a0[k] = r[R_ALPHA0]; b0[k] = r[R_BETA0]; done[k] = r[R_ITERS]; code[k] = r[R_CODE];
    if (iteration == 0) {                                         // the frame begins: what the last frame ended with
      a0[k] = r[R_ALPHA]; b0[k] = r[R_BETA]; done[k] = 0.0; code[k] = 0.0;
    }
    alpha[k] = a0[k];
    beta[k] = b0[k];
  }
  double al = 0.0, be = 0.0;
  const double frame = solve(S, S[VALID], min_valid, var_min, al, be);
  if (frame == 0.0) {
    alpha[0] = al;
    beta[0] = be;
    done[0] = done[0] + 1.0;
  } else {
    code[0] = frame;
  }
#pragma unroll
  for (int k = 1; k < REGS; ++k) {
    double ak = 0.0, bk = 0.0;
    if (code[k] == 0.0) code[k] = solve(S + k * PER, S[VALID], min_valid, var_min, ak, bk);   // a channel with a code keeps it
    if (frame != 0.0) continue;                                   // the frame's fit has ended: every regression is at its start
    if (code[k] == 0.0) {
      alpha[k] = ak;
      beta[k] = bk;
      done[k] = done[k] + 1.0;
    } else {                                                      // the channel follows the grey
      alpha[k] = alpha[0];
      beta[k] = beta[0];
    }
  }
#pragma unroll
  for (int k = 0; k < REGS; ++k) {
    double* r = state + k * REG;
    r[R_ALPHA] = alpha[k]; r[R_BETA] = beta[k]; r[R_ALPHA0] = a0[k]; r[R_BETA0] = b0[k]; r[R_CODE] = code[k]; r[R_ITERS] = done[k];
  }
  state[S_FRAME] = frame;
}

// one thread per pixel: the three channels, both layouts
__global__ void __launch_bounds__(NT) apply_kernel(const float* __restrict__ color, int64_t n, const double* __restrict__ state,
                                                   float* __restrict__ out_chw, float* __restrict__ out_hwc) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float alpha = (float)state[(c + 1) * REG + R_ALPHA], beta = (float)state[(c + 1) * REG + R_BETA];
    float v = alpha * color[c * n + i];
    v = v + beta;
    v = fminf(fmaxf(v, 0.f), 1.f);                               // a NaN becomes 0
    out_chw[c * n + i] = v;
    out_hwc[3 * i + c] = v;
  }
}

static bool size_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && (int64_t)H * W < 0x80000000LL; }

}  // namespace rtgs_white_balance_k

extern "C" {

using namespace rtgs_white_balance_k;

size_t rtgs_white_balance_scratch_bytes(int32_t H, int32_t W) {
  if (!size_ok(H, W)) return 0;
  return (size_t)(((int64_t)H * W + CHUNK - 1) / CHUNK) * OUT * sizeof(double);
}

int rtgs_white_balance_fit(const float* src_color_chw, const float* src_depth, const float* dst_color_chw, const float* dst_depth,
                           const float* T_map, int32_t H, int32_t W, int32_t iteration, float huber, float cut, float depth_gate,
                           float t_gate, float src_lo, float src_hi, float dst_lo, float dst_hi, double var_min, int64_t min_valid,
                           double* state, void* scratch, void* stream) {
  if (!size_ok(H, W) || iteration < 0) return -1;
  if (!src_color_chw || !src_depth || !dst_color_chw || !dst_depth || !T_map || !state || !scratch) return -1;
  if (!(huber > 0.f) || !(cut >= 1.f) || !(depth_gate >= 0.f) || !(src_lo <= src_hi) || !(dst_lo <= dst_hi) || !(var_min >= 0.0) ||
      min_valid < 1)                                                               // or NaN
    return -1;
  if (t_gate != t_gate) return -1;
  const int64_t n = (int64_t)H * W;
  const int64_t chunks = (n + CHUNK - 1) / CHUNK;                                  // < 2^21
  Gates g;
  g.huber = huber;
  g.cutoff = cut * huber;                                                          // one rounded float32 product
  g.depth_gate = depth_gate; g.t_gate = t_gate;
  g.src_lo = src_lo; g.src_hi = src_hi; g.dst_lo = dst_lo; g.dst_hi = dst_hi;
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)scratch;
  hipLaunchKernelGGL(chunks_kernel, dim3((unsigned)chunks), dim3(NT), 0, s, src_color_chw, src_depth, dst_color_chw, dst_depth,
                     T_map, n, (int)iteration, g, (const double*)state, partial);
  hipLaunchKernelGGL(total_kernel, dim3(1), dim3(NT), 0, s, (const double*)partial, chunks, (int)iteration, var_min,
                     (double)min_valid, state);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_white_balance_apply(const float* color_chw, int32_t H, int32_t W, const double* state, float* out_chw, float* out_hwc,
                             void* stream) {
  if (!size_ok(H, W) || !color_chw || !state || !out_chw || !out_hwc) return -1;
  if (out_chw == color_chw || out_hwc == color_chw) return -1;         // the raw colour stays what it is
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(apply_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, color_chw, n, state,
                     out_chw, out_hwc);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
