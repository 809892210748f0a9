// gfx950 kernels + C ABI of the map-quality evaluation (include/rtgs_slam.h, "evaluation"): the picture metrics of
// SLAM/eval.py::eval_picture (PSNR, MS-SSIM, colour L1, depth L1, valid-pixel ratio) and the per-point reduction behind
// eval_pcd's accuracy / completion / precision / recall (the nearest-neighbour search itself is rtgs_knn3_build_ref /
// rtgs_knn3_query_built).
//
// Design:
//  * Every result is bitwise reproducible run to run.  No float atomics anywhere: each kernel writes one partial per
//    workgroup into a slab (its grid depends only on the image / point count), a single-workgroup kernel reduces every slab
//    column in a fixed order.  All accumulation is float64: per thread, in the LDS tree of a workgroup and across slabs.
//  * Per-pixel sums: ONE grid-stride pass over render, gt, depth, gt depth and depth index (36 B per pixel).
//  * MS-SSIM, per level: one tiled kernel per (32 x 16 output tile, channel).  x and y of the tile plus its 10-pixel halo are
//    staged in LDS as float32; the 11-tap Gaussian is applied separably in float64 to the five maps x, y, x^2, y^2, xy
//    (horizontal pass into LDS, vertical pass in registers), so the VALID window of a level needs no second read of
//    global memory, and the float64 arithmetic keeps the sigma = f(x^2) - mu^2 cancellations exact enough for a 1e-5 bound.
//    The tile's sums of cs and ssim go to the level's slab.  The 2 x 2 average pooling to the next level is a small
//    separate kernel (float32, as torch's avg_pool2d; odd axes padded by one zero in front, divisor 4).
//  * The final kernel forms the means, the per-channel products of powers and the channel mean, and writes the float64
//    result vector; the host reads it once.
#include "../../include/rtgs_slam.h"
#include <hip/hip_runtime.h>
#include <math.h>

namespace rtgs_eval {

constexpr int NT = 256;                        // threads per workgroup of every kernel here
constexpr int SUM_BLOCKS = 512;                // cap of the per-pixel pass's grid (grid-stride beyond)
constexpr int NN_BLOCKS = 1024;                // cap of the per-point pass's grid
constexpr int SUM_COLS = 8;                    // se_r se_g se_b l1 depth_l1 valid (2 spare)
constexpr int LEVELS = 5;
constexpr int WIN = 11, HALO = WIN - 1;
constexpr int TW = 32, TH = 16;                // output tile of the level kernel
constexpr int SW = TW + HALO, SH = TH + HALO;  // staged input tile
constexpr int MAXK = RTGS_EVAL_MAX_THRESHOLDS;

struct Window { double g[WIN]; };

struct Plan {
  int h[LEVELS], w[LEVELS], tx[LEVELS], ty[LEVELS];
  int n_sum;                                   // blocks of the per-pixel pass
  bool ms;                                     // the pyramid exists (smaller side > 160)
  size_t off_sums, off_lvl[LEVELS], off_img[LEVELS], bytes;
};

__host__ __device__ inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

inline Plan make_plan(int H, int W) {
  Plan p{};
  const long long n = (long long)H * W;
  p.n_sum = (int)((n + NT - 1) / NT < SUM_BLOCKS ? (n + NT - 1) / NT : SUM_BLOCKS);
  if (p.n_sum < 1) p.n_sum = 1;
  p.ms = (H < W ? H : W) > RTGS_EVAL_MS_SSIM_MIN_SIDE;
  size_t o = 0;
  p.off_sums = o;
  o = align256(o + sizeof(double) * SUM_COLS * p.n_sum);
  if (!p.ms) { p.bytes = o; return p; }
  int h = H, w = W;
  for (int l = 0; l < LEVELS; ++l) {
    p.h[l] = h; p.w[l] = w;
    p.tx[l] = (w - HALO + TW - 1) / TW;
    p.ty[l] = (h - HALO + TH - 1) / TH;
    h = (h + (h & 1)) / 2;
    w = (w + (w & 1)) / 2;
  }
  for (int l = 0; l < LEVELS; ++l) {
    p.off_lvl[l] = o;
    o = align256(o + sizeof(double) * 2 * 3 * (size_t)p.tx[l] * p.ty[l]);
  }
  p.off_img[0] = 0;                            // level 0 is the caller's render / gt
  for (int l = 1; l < LEVELS; ++l) {
    p.off_img[l] = o;                          // x then y, each [3, h, w] float32
    o = align256(o + sizeof(float) * 2 * 3 * (size_t)p.h[l] * p.w[l]);
  }
  p.bytes = o;
  return p;
}

// Sum of v over the workgroup in a fixed tree order; every thread gets the result.  s: NT doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* s) {
  s[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

// Column `col` of a [rows, ncol] slab, summed by one workgroup: thread t takes rows t, t + NT, ... in order, then the tree.
__device__ __forceinline__ double slab_sum(const double* slab, int rows, int ncol, int col, double* s) {
  double a = 0.0;
  for (int r = threadIdx.x; r < rows; r += NT) a += slab[(size_t)r * ncol + col];
  return block_sum(a, s);
}

// ------------------------------------------------------------------------------------------------ per-pixel sums
__global__ void __launch_bounds__(NT) picture_sums_kernel(const float* __restrict__ render, const float* __restrict__ gt,
                                                          const float* __restrict__ depth, const float* __restrict__ gt_depth,
                                                          const int32_t* __restrict__ didx, int n, float min_d, float max_d,
                                                          double* __restrict__ slab) {
  __shared__ double s[NT];
  double se0 = 0.0, se1 = 0.0, se2 = 0.0, l1 = 0.0, dl1 = 0.0, cnt = 0.0;
  for (int p = blockIdx.x * NT + threadIdx.x; p < n; p += gridDim.x * NT) {
    // differences in float32, as the reference's torch expressions; squares and sums in float64
    const float d0 = gt[p] - render[p];
    const float d1 = gt[(size_t)n + p] - render[(size_t)n + p];
    const float d2 = gt[2 * (size_t)n + p] - render[2 * (size_t)n + p];
    se0 += (double)d0 * d0;
    se1 += (double)d1 * d1;
    se2 += (double)d2 * d2;
    l1 += (double)fabsf(d0);
    l1 += (double)fabsf(d1);
    l1 += (double)fabsf(d2);
    float g = gt_depth[p];
    if (!(g > min_d && g < max_d)) g = 0.f;    // outside the open range (NaN included) -> 0, eval.py:80-82
    if (didx[p] != -1 && g != 0.f) {
      dl1 += (double)fabsf(depth[p] - g);
      cnt += 1.0;
    }
  }
  const double v[6] = {se0, se1, se2, l1, dl1, cnt};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double t = block_sum(v[k], s);
    if (threadIdx.x == 0) slab[(size_t)blockIdx.x * SUM_COLS + k] = t;
  }
}

// ------------------------------------------------------------------------------------------------ MS-SSIM levels
// grid (tx, ty, 3 channels).  Output pixel (oy, ox) of the VALID window is the window whose top-left input pixel is (oy, ox).
__global__ void __launch_bounds__(NT) ssim_level_kernel(const float* __restrict__ x, const float* __restrict__ y, int h, int w,
                                                        Window win, double* __restrict__ slab) {
  __shared__ float sx[SH][SW + 1], sy[SH][SW + 1];
  __shared__ double hp[5][SH][TW];             // horizontally filtered x, y, xx, yy, xy
  __shared__ double s[NT];
  const int c = blockIdx.z;
  const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
  const int oh = h - HALO, ow = w - HALO;
  const float* xc = x + (size_t)c * h * w;
  const float* yc = y + (size_t)c * h * w;
  for (int i = threadIdx.x; i < SH * SW; i += NT) {
    const int r = i / SW, q = i - r * SW;
    const int gy = oy0 + r, gx = ox0 + q;
    const bool in = gy < h && gx < w;          // beyond the image: never reaches a valid output
    sx[r][q] = in ? xc[(size_t)gy * w + gx] : 0.f;
    sy[r][q] = in ? yc[(size_t)gy * w + gx] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SH * TW; i += NT) {
    const int r = i / TW, q = i - r * TW;
    double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
    for (int k = 0; k < WIN; ++k) {
      const double xv = sx[r][q + k], yv = sy[r][q + k], g = win.g[k];
      a += g * xv;
      b += g * yv;
      aa += g * (xv * xv);
      bb += g * (yv * yv);
      ab += g * (xv * yv);
    }
    hp[0][r][q] = a; hp[1][r][q] = b; hp[2][r][q] = aa; hp[3][r][q] = bb; hp[4][r][q] = ab;
  }
  __syncthreads();
  constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
  double cs_acc = 0.0, ss_acc = 0.0;
  for (int i = threadIdx.x; i < TH * TW; i += NT) {
    const int r = i / TW, q = i - r * TW;
    if (oy0 + r < oh && ox0 + q < ow) {
      double mx = 0.0, my = 0.0, fxx = 0.0, fyy = 0.0, fxy = 0.0;
#pragma unroll
      for (int k = 0; k < WIN; ++k) {
        const double g = win.g[k];
        mx += g * hp[0][r + k][q];
        my += g * hp[1][r + k][q];
        fxx += g * hp[2][r + k][q];
        fyy += g * hp[3][r + k][q];
        fxy += g * hp[4][r + k][q];
      }
      const double sxx = fxx - mx * mx, syy = fyy - my * my, sxy = fxy - mx * my;
      const double cs = (2.0 * sxy + C2) / (sxx + syy + C2);
      cs_acc += cs;
      ss_acc += (2.0 * mx * my + C1) / (mx * mx + my * my + C1) * cs;
    }
  }
  const int blk = blockIdx.y * gridDim.x + blockIdx.x, nblk = gridDim.x * gridDim.y;
  const double tc = block_sum(cs_acc, s), ts = block_sum(ss_acc, s);
  if (threadIdx.x == 0) {
    slab[((size_t)c * nblk + blk) * 2 + 0] = tc;
    slab[((size_t)c * nblk + blk) * 2 + 1] = ts;
  }
}

// avg_pool2d(kernel 2, stride 2, padding (h % 2, w % 2), count_include_pad) of x and y, [3, h, w] -> [3, h2, w2]
__global__ void __launch_bounds__(NT) pool2_kernel(const float* __restrict__ x, const float* __restrict__ y, int h, int w, int h2,
                                                   int w2, float* __restrict__ x2, float* __restrict__ y2) {
  const int per = h2 * w2, total = 3 * per;
  const int ph = h & 1, pw = w & 1;
  for (int i = blockIdx.x * NT + threadIdx.x; i < total; i += gridDim.x * NT) {
    const int c = i / per, rem = i - c * per;
    const int oy = rem / w2, ox = rem - oy * w2;
    const int r0 = 2 * oy - ph, c0 = 2 * ox - pw;         // r0 + 1 <= h - 1 and c0 + 1 <= w - 1 always; only -1 is padding
    const float* xc = x + (size_t)c * h * w;
    const float* yc = y + (size_t)c * h * w;
    float sxv = 0.f, syv = 0.f;
#pragma unroll
    for (int dr = 0; dr < 2; ++dr)
#pragma unroll
      for (int dc = 0; dc < 2; ++dc) {
        const int rr = r0 + dr, cc = c0 + dc;
        if (rr >= 0 && cc >= 0) {
          sxv += xc[(size_t)rr * w + cc];
          syv += yc[(size_t)rr * w + cc];
        }
      }
    x2[i] = sxv / 4.f;
    y2[i] = syv / 4.f;
  }
}

// ------------------------------------------------------------------------------------------------ final reduction
struct FinalArgs {
  const double* sums;
  const double* lvl[LEVELS];
  int n_sum, nblk[LEVELS];
  double npix, nvalid[LEVELS];
  int ms;
};

__global__ void __launch_bounds__(NT) picture_final_kernel(FinalArgs a, double* __restrict__ out) {
  __shared__ double s[NT];
  double tot[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) tot[k] = slab_sum(a.sums, a.n_sum, SUM_COLS, k, s);
  double cs[LEVELS][3], ss[LEVELS][3];
#pragma unroll
  for (int l = 0; l < LEVELS; ++l)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (a.ms) {
        const double* base = a.lvl[l] + (size_t)c * a.nblk[l] * 2;
        cs[l][c] = slab_sum(base, a.nblk[l], 2, 0, s) / a.nvalid[l];
        ss[l][c] = slab_sum(base, a.nblk[l], 2, 1, s) / a.nvalid[l];
      } else {
        cs[l][c] = ss[l][c] = NAN;
      }
    }
  if (threadIdx.x != 0) return;
  double psnr = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double mse = tot[c] / a.npix;
    out[RTGS_EVAL_OUT_MSE + c] = mse;
    psnr += 20.0 * log10(1.0 / sqrt(mse));                // mse = 0 -> +inf, as torch
  }
  out[RTGS_EVAL_OUT_PSNR] = psnr / 3.0;
  out[RTGS_EVAL_OUT_COLOR_L1] = tot[3] / (3.0 * a.npix);
  out[RTGS_EVAL_OUT_DEPTH_L1] = tot[4] / tot[5];          // 0 / 0 = NaN without a valid pixel, as the reference's mean
  out[RTGS_EVAL_OUT_VALID_RATIO] = tot[5] / a.npix;
  out[RTGS_EVAL_OUT_VALID_COUNT] = tot[5];
  const double wts[LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  double ms = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double prod = 1.0;
#pragma unroll
    for (int l = 0; l < LEVELS; ++l) {
      const double v = l < LEVELS - 1 ? cs[l][c] : ss[l][c];
      prod *= pow(v > 0.0 ? v : 0.0, wts[l]);             // relu, then the level's weight
      out[RTGS_EVAL_OUT_CS + 3 * l + c] = cs[l][c];
      out[RTGS_EVAL_OUT_SSIM + 3 * l + c] = ss[l][c];
    }
    ms += prod;
  }
  out[RTGS_EVAL_OUT_MS_SSIM] = a.ms ? ms / 3.0 : NAN;
}

// ------------------------------------------------------------------------------------------------ nearest-neighbour stats
__global__ void __launch_bounds__(NT) nn_stats_kernel(const float* __restrict__ dist2, int n, const double* __restrict__ thr, int k,
                                                      double* __restrict__ slab) {
  __shared__ double s[NT];
  __shared__ double st[MAXK];
  if ((int)threadIdx.x < k) st[threadIdx.x] = thr[threadIdx.x];
  __syncthreads();
  double dsum = 0.0;
  uint32_t cnt[MAXK];
#pragma unroll
  for (int j = 0; j < MAXK; ++j) cnt[j] = 0;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    const double d = sqrt((double)dist2[(size_t)i * 3]);   // column 0: the nearest neighbour
    dsum += d;
#pragma unroll
    for (int j = 0; j < MAXK; ++j)
      if (j < k) cnt[j] += d < st[j] ? 1u : 0u;
  }
  const int ncol = 1 + k;
  const double t0 = block_sum(dsum, s);
  if (threadIdx.x == 0) slab[(size_t)blockIdx.x * ncol] = t0;
#pragma unroll
  for (int j = 0; j < MAXK; ++j) {
    if (j < k) {                                            // k is uniform over the workgroup
      const double t = block_sum((double)cnt[j], s);
      if (threadIdx.x == 0) slab[(size_t)blockIdx.x * ncol + 1 + j] = t;
    }
  }
}

__global__ void __launch_bounds__(NT) nn_final_kernel(const double* __restrict__ slab, int rows, int ncol, double* __restrict__ out) {
  __shared__ double s[NT];
  for (int c = 0; c < ncol; ++c) {
    const double t = slab_sum(slab, rows, ncol, c, s);
    if (threadIdx.x == 0) out[c] = t;
  }
}

inline int nn_blocks(int n) { return (n + NT - 1) / NT < NN_BLOCKS ? (n + NT - 1) / NT : NN_BLOCKS; }

}  // namespace rtgs_eval

using namespace rtgs_eval;

#define EVAL_TRY(expr)                       \
  do {                                       \
    if ((expr) != hipSuccess) return -2;     \
  } while (0)

extern "C" {

size_t rtgs_eval_picture_scratch_bytes(int32_t H, int32_t W) {
  if (H <= 0 || W <= 0) return 0;
  return make_plan(H, W).bytes;
}

int rtgs_eval_picture(const float* render, const float* gt_color, const float* depth, const float* gt_depth,
                      const int32_t* depth_index, int32_t H, int32_t W, float min_depth, float max_depth, int32_t with_ms_ssim,
                      void* scratch, double* out, void* stream) {
  if (!render || !gt_color || !depth || !gt_depth || !depth_index || !scratch || !out || H <= 0 || W <= 0) return -1;
  if ((long long)H * W > 0x7fffffffLL / 3) return -1;
  const Plan p = make_plan(H, W);
  if (with_ms_ssim && !p.ms) return -1;                     // pytorch_msssim asserts smaller side > 160
  hipStream_t st = (hipStream_t)stream;
  char* sc = (char*)scratch;
  double* sums = (double*)(sc + p.off_sums);
  const int n = H * W;
  hipLaunchKernelGGL(picture_sums_kernel, dim3(p.n_sum), dim3(NT), 0, st, render, gt_color, depth, gt_depth, depth_index, n,
                     min_depth, max_depth, sums);
  EVAL_TRY(hipGetLastError());
  FinalArgs fa{};
  fa.sums = sums;
  fa.n_sum = p.n_sum;
  fa.npix = (double)n;
  fa.ms = with_ms_ssim ? 1 : 0;
  if (with_ms_ssim) {
    Window win;
    double tot = 0.0;
    for (int k = 0; k < WIN; ++k) tot += (win.g[k] = exp(-double((k - 5) * (k - 5)) / 4.5));   // sigma 1.5
    for (int k = 0; k < WIN; ++k) win.g[k] /= tot;
    const float* xs = render;
    const float* ys = gt_color;
    for (int l = 0; l < LEVELS; ++l) {
      double* slab = (double*)(sc + p.off_lvl[l]);
      hipLaunchKernelGGL(ssim_level_kernel, dim3(p.tx[l], p.ty[l], 3), dim3(NT), 0, st, xs, ys, p.h[l], p.w[l], win, slab);
      EVAL_TRY(hipGetLastError());
      fa.lvl[l] = slab;
      fa.nblk[l] = p.tx[l] * p.ty[l];
      fa.nvalid[l] = (double)(p.h[l] - HALO) * (p.w[l] - HALO);
      if (l + 1 < LEVELS) {
        float* x2 = (float*)(sc + p.off_img[l + 1]);
        float* y2 = x2 + (size_t)3 * p.h[l + 1] * p.w[l + 1];
        const int total = 3 * p.h[l + 1] * p.w[l + 1];
        const int g = (total + NT - 1) / NT < 2048 ? (total + NT - 1) / NT : 2048;
        hipLaunchKernelGGL(pool2_kernel, dim3(g), dim3(NT), 0, st, xs, ys, p.h[l], p.w[l], p.h[l + 1], p.w[l + 1], x2, y2);
        EVAL_TRY(hipGetLastError());
        xs = x2;
        ys = y2;
      }
    }
  }
  hipLaunchKernelGGL(picture_final_kernel, dim3(1), dim3(NT), 0, st, fa, out);
  EVAL_TRY(hipGetLastError());
  return 0;
}

size_t rtgs_eval_nn_stats_scratch_bytes(int32_t N, int32_t k) {
  if (N <= 0 || k < 0 || k > MAXK) return 0;
  return sizeof(double) * (size_t)nn_blocks(N) * (1 + k);
}

int rtgs_eval_nn_stats(const float* dist2, int32_t N, const double* thresholds, int32_t k, void* scratch, double* out, void* stream) {
  if (!dist2 || !scratch || !out || N <= 0 || k < 0 || k > MAXK || (k > 0 && !thresholds)) return -1;
  if ((long long)N * 3 > 0x7fffffffLL) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int nb = nn_blocks(N);
  double* slab = (double*)scratch;
  hipLaunchKernelGGL(nn_stats_kernel, dim3(nb), dim3(NT), 0, st, dist2, N, thresholds, k, slab);
  EVAL_TRY(hipGetLastError());
  hipLaunchKernelGGL(nn_final_kernel, dim3(1), dim3(NT), 0, st, (const double*)slab, nb, 1 + k, out);
  EVAL_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
