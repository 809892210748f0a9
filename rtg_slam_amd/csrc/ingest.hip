// gfx950 kernel + C ABI of the frame ingest (include/rtgs_slam.h, "frame ingest"): the raw bytes of one decoded RGB-D frame
// (u16 depth [Hd,Wd], u8 colour [Hd,Wd,3|4]) -> the cropped float32 maps the SLAM loop consumes (depth [H,W] in metres,
// colour [3,H,W] in 0..1), H = Hd - 2 crop, W = Wd - 2 crop; and the same with a resize after the crop ("resized ingest"
// below).
//
// The float chain is the reference's, one correctly rounded float32 operation per step:
//   depth  scene/dataset_readers.py:890-891   d = f32(raw) / f32(depth_scale)        (numpy float32)
//          utils/general_utils.py:43-49       d = d / 255                             (PILtoTorch, torch on the CPU)
//          SLAM/multiprocess/tracker.py:97-101 d = d * 255                            (map_preprocess, on the GPU)
//   colour utils/general_utils.py:43-49       c = f32(u8) / 255, HWC -> CHW, alpha dropped
// This file is built without fast-math and with -ffp-contract=off (Makefile EXTRA_ingest): the divisions stay IEEE
// divisions (v_div_scale / v_div_fmas / v_div_fixup), (d / 255) * 255 is not folded and nothing is contracted.
//
// Memory-bound: ~17 B per 1200 x 680 output pixel.  Each thread handles a quad of 4 output pixels of one row; when the quad is
// whole and every address it touches is aligned (the common case: W, Wd and crop multiples of 4), the loads are one 8-B
// depth load and one 16-B (RGBA) or three 4-B (RGB) colour loads, the stores one 16-B store per output plane; otherwise
// the quad is handled pixel by pixel.  Grid-stride over the quads.
#include "../../include/rtgs_slam.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtgs_ingest {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;

__device__ __forceinline__ float depth_chain(uint32_t raw, float scale) {
  float d = (float)raw / scale;
  d = d / 255.0f;
  return d * 255.0f;
}

__device__ __forceinline__ float color_chain(uint32_t c) { return (float)c / 255.0f; }

template <int CH>
__global__ void __launch_bounds__(NT) ingest_kernel(const uint16_t* __restrict__ depth_raw, const uint8_t* __restrict__ color_raw,
                                                     int Wd, int crop, int H, int W, float scale, int aligned,
                                                     float* __restrict__ depth_out, float* __restrict__ color_out) {
  const int qw = (W + 3) >> 2;
  const long long nq = (long long)H * qw;
  const long long plane = (long long)H * W;
  for (long long q = (long long)blockIdx.x * NT + threadIdx.x; q < nq; q += (long long)gridDim.x * NT) {
    const int y = (int)(q / qw);
    const int x0 = (int)(q - (long long)y * qw) * 4;
    const long long in0 = (long long)(y + crop) * Wd + (x0 + crop);      // input pixel of output (y, x0)
    const long long out0 = (long long)y * W + x0;
    if (aligned && x0 + 4 <= W) {
      // aligned != 0 promises: Wd, crop, W multiples of 4 and 16-B aligned bases -> every vector access below is aligned
      const uint2 dr = *reinterpret_cast<const uint2*>(depth_raw + in0);
      const uint32_t r[4] = {dr.x & 0xffffu, dr.x >> 16, dr.y & 0xffffu, dr.y >> 16};
      uint32_t c[4][3];
      if (CH == 4) {
        const uint4 cr = *reinterpret_cast<const uint4*>(color_raw + in0 * 4);
        const uint32_t w[4] = {cr.x, cr.y, cr.z, cr.w};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          c[p][0] = w[p] & 0xffu; c[p][1] = (w[p] >> 8) & 0xffu; c[p][2] = (w[p] >> 16) & 0xffu;
        }
      } else {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(color_raw + in0 * 3);
        const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
        const uint32_t b[12] = {w0 & 0xffu, (w0 >> 8) & 0xffu, (w0 >> 16) & 0xffu, w0 >> 24,
                                w1 & 0xffu, (w1 >> 8) & 0xffu, (w1 >> 16) & 0xffu, w1 >> 24,
                                w2 & 0xffu, (w2 >> 8) & 0xffu, (w2 >> 16) & 0xffu, w2 >> 24};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          c[p][0] = b[3 * p]; c[p][1] = b[3 * p + 1]; c[p][2] = b[3 * p + 2];
        }
      }
      *reinterpret_cast<float4*>(depth_out + out0) =
          make_float4(depth_chain(r[0], scale), depth_chain(r[1], scale), depth_chain(r[2], scale), depth_chain(r[3], scale));
#pragma unroll
      for (int k = 0; k < 3; ++k)
        *reinterpret_cast<float4*>(color_out + k * plane + out0) =
            make_float4(color_chain(c[0][k]), color_chain(c[1][k]), color_chain(c[2][k]), color_chain(c[3][k]));
    } else {
      const int n = W - x0 < 4 ? W - x0 : 4;
      for (int p = 0; p < n; ++p) {
        depth_out[out0 + p] = depth_chain(depth_raw[in0 + p], scale);
        const uint8_t* px = color_raw + (in0 + p) * CH;
#pragma unroll
        for (int k = 0; k < 3; ++k) color_out[k * plane + out0 + p] = color_chain(px[k]);
      }
    }
  }
}

}  // namespace rtgs_ingest

// ---- resized ingest ---------------------------------------------------------------------------------------------------------
// rtgs_ingest_rgbd_resized: the same frame, resized to Ho x Wo after the crop as utils/camera_utils.py:22-74 (loadCam) does
// with PIL: colour Image.resize(BILINEAR) on the u8 image, then / 255; depth Image.resize(NEAREST) on the float image, i.e.
// a source-pixel pick followed by depth_chain.  Pillow's 8-bit resampler is integer arithmetic: a horizontal pass, then a
// vertical pass on the ROUNDED u8 result of the first; each pass sum = 2^21 + sum_j coeff[j] * src[start + j], >> 22, clipped
// to 0..255.  The windows and the 22-bit coefficients (and the nearest source index) per output column and row come from the
// host, computed in float64 as Pillow does (datasets.resample_tables / nearest_indices): nothing here computes an index in
// floating point.  An RGBA image is resampled as Image.resize does it: colours premultiplied by alpha on the way in
// (t = c a + 128; ((t >> 8) + t) >> 8), alpha resampled beside them, colours divided by the resampled alpha on the way out
// (255 c / a, clipped; left as they are when a is 0 or 255).
//
// One launch, no intermediate image in global memory.  A workgroup owns RS_TW x th output pixels.  Phase 1: its 256 threads
// resample horizontally the source rows [ybase, yend) that the tile's vertical windows cover, one packed u8x4 per pixel
// into LDS (rows[r][RS_TW]), four rows at a time so that their byte loads overlap (the loop is bound by load latency, not by
// bytes), and the tile's vertical coefficients beside them.  Phase 2: thread (ty, q) owns output row y0 + ty, columns x0 + 4q .. +3: per window row one
// 16-B LDS read (the 16 lanes of a ds_read_b128 group read 256 contiguous bytes: no bank conflict), integer multiply-adds,
// the second rounding, the float chain, and one 16-B store per plane when Wo is a multiple of 4 and the planes are
// aligned.  th is 16 unless the rows of a 16-row tile do not fit 64 KiB of LDS (reduction factors above ~14), then the
// largest of 8, 4, 2, 1 that fits; when one output row's window does not fit either, the entry point returns -1.  A small
// output also gets flatter tiles (down to 2 rows) until there is a tile per CU.
// Table values come from device memory and cannot be checked on the host, so every index derived from them is clamped to
// the buffer it addresses: wrong tables give wrong pixels, never an access out of bounds.
namespace rtgs_ingest {

constexpr int RS_TW = 64;                 // tile width in output pixels (16 quads)
constexpr int RS_TH = 16;                 // tile height at most: 16 x 16 quads = NT threads
constexpr int RS_RU = 4;                  // source rows a thread resamples at a time in phase 1
constexpr int RS_BITS = 22;               // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int RS_LDS_MAX = 64 * 1024;
constexpr int RS_MIN_TILES = 256;         // the MI355X has 256 CUs

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// Pillow's clip8.  The weights are non-negative, so a sum is never negative and only the upper bound can bind: a logical
// shift and an unsigned minimum.  (Written as a signed shift clamped to 0..255, two of these packed into one word select
// gfx950's v_ashr_pk_u8_i32, whose result the compiler ORs with the other bytes as if the upper half of the register had
// been cleared; on the MI355X it was not, and every row after a thread's first came out wrong.)
__device__ __forceinline__ uint32_t clip8(int acc) { const uint32_t v = (uint32_t)acc >> RS_BITS; return v < 255u ? v : 255u; }
__device__ __forceinline__ uint32_t muldiv255(uint32_t a, uint32_t b) { const uint32_t t = a * b + 128u; return ((t >> 8) + t) >> 8; }

struct ResizeTab {                        // views into the packed table buffer (rtgs_slam.h)
  const int32_t *x_start, *x_len, *x_near, *y_start, *y_len, *y_near, *x_coeff, *y_coeff;
};

template <int CH>
__global__ void __launch_bounds__(NT) ingest_resized_kernel(const uint16_t* __restrict__ depth_raw, const uint8_t* __restrict__ color_raw,
                                                             int Wd, int crop, int Hc, int Wc, int Ho, int Wo, float scale,
                                                             const int32_t* __restrict__ tab, int kx, int ky, int th, int R, int vec,
                                                             float* __restrict__ depth_out, float* __restrict__ color_out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rows[];            // [R][RS_TW] packed u8 x 4, then int32 [th][ky]
  int32_t* ycoef = reinterpret_cast<int32_t*>(rows + R * RS_TW);
  ResizeTab t;
  t.x_start = tab; t.x_len = tab + Wo; t.x_near = tab + 2 * Wo;
  t.y_start = tab + 3 * Wo; t.y_len = t.y_start + Ho; t.y_near = t.y_start + 2 * Ho;
  t.x_coeff = t.y_start + 3 * Ho; t.y_coeff = t.x_coeff + (long long)Wo * kx;
  const int x0 = blockIdx.x * RS_TW, y0 = blockIdx.y * th;
  const int ylast = (y0 + th < Ho ? y0 + th : Ho) - 1;
  const int ybase = clampi(t.y_start[y0], 0, Hc - 1);
  int nrows = clampi(t.y_start[ylast], 0, Hc - 1) + clampi(t.y_len[ylast], 0, ky) - ybase;
  nrows = clampi(nrows, 0, R);
  if (ybase + nrows > Hc) nrows = Hc - ybase;

  // phase 1: horizontal pass of source rows ybase .. ybase + nrows - 1 for this tile's columns.  NT is a multiple of RS_TW,
  // so a thread keeps its column: window start and length are loaded once.
  {
    const int tx = threadIdx.x & (RS_TW - 1);
    const int x = x0 + tx;
    if (x < Wo) {
      const int xs = clampi(t.x_start[x], 0, Wc - 1);
      int xl = clampi(t.x_len[x], 0, kx);
      if (xs + xl > Wc) xl = Wc - xs;
      const int32_t* kc = t.x_coeff + (long long)x * kx;
      // RS_RU rows at a time: their byte loads are independent, so RS_RU x CH loads are in flight per tap instead of CH
      for (int r0 = threadIdx.x / RS_TW; r0 < nrows; r0 += RS_RU * (NT / RS_TW)) {
        const uint8_t* px[RS_RU];
        int a[RS_RU][4];
#pragma unroll
        for (int u = 0; u < RS_RU; ++u) {
          const int r = r0 + u * (NT / RS_TW) < nrows ? r0 + u * (NT / RS_TW) : nrows - 1;      // beyond the tile: a row again
          px[u] = color_raw + ((long long)(ybase + r + crop) * Wd + (crop + xs)) * CH;
          a[u][0] = a[u][1] = a[u][2] = a[u][3] = 1 << (RS_BITS - 1);
        }
        for (int j = 0; j < xl; ++j) {
          const int k = kc[j];
#pragma unroll
          for (int u = 0; u < RS_RU; ++u) {
            uint32_t c0 = px[u][j * CH], c1 = px[u][j * CH + 1], c2 = px[u][j * CH + 2];
            if (CH == 4) {
              const uint32_t al = px[u][j * CH + 3];
              c0 = muldiv255(c0, al); c1 = muldiv255(c1, al); c2 = muldiv255(c2, al);
              a[u][3] += k * (int)al;
            }
            a[u][0] += k * (int)c0; a[u][1] += k * (int)c1; a[u][2] += k * (int)c2;
          }
        }
#pragma unroll
        for (int u = 0; u < RS_RU; ++u) {
          const int r = r0 + u * (NT / RS_TW);
          if (r < nrows)
            rows[r * RS_TW + tx] = clip8(a[u][0]) | (clip8(a[u][1]) << 8) | (clip8(a[u][2]) << 16) | (CH == 4 ? clip8(a[u][3]) << 24 : 0u);
        }
      }
    }
  }
  // the tile's vertical coefficients (th x ky, contiguous in the table) into LDS, so that phase 2 reads no global table
  {
    const long long first = (long long)y0 * ky, total = (long long)Ho * ky;
    for (int i = threadIdx.x; i < th * ky; i += NT) ycoef[i] = first + i < total ? t.y_coeff[first + i] : 0;
  }
  __syncthreads();

  // phase 2: vertical pass from LDS, float chain, planar stores
  const int q = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int y = y0 + ty, xq = x0 + 4 * q;
  if (ty >= th || y >= Ho || xq >= Wo) return;
  const int rel0 = clampi(t.y_start[y], 0, Hc - 1) - ybase;
  int yl = clampi(t.y_len[y], 0, ky);
  if (rel0 < 0) yl = 0;
  if (rel0 + yl > nrows) yl = nrows - rel0 > 0 ? nrows - rel0 : 0;
  const int32_t* kc = ycoef + ty * ky;
  int acc[4][CH];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int k = 0; k < CH; ++k) acc[p][k] = 1 << (RS_BITS - 1);
  for (int j = 0; j < yl; ++j) {
    const int k = kc[j];
    const uint4 v = *reinterpret_cast<const uint4*>(rows + (rel0 + j) * RS_TW + 4 * q);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[p][c] += k * (int)((w[p] >> (8 * c)) & 0xffu);
  }
  const int n = Wo - xq < 4 ? Wo - xq : 4;
  float dep[4], col[3][4];
  const long long drow = (long long)(clampi(t.y_near[y], 0, Hc - 1) + crop) * Wd + crop;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int xx = p < n ? xq + p : xq;                                          // a partial quad repeats its first pixel
    dep[p] = depth_chain(depth_raw[drow + clampi(t.x_near[xx], 0, Wc - 1)], scale);
    uint32_t c[3] = {clip8(acc[p][0]), clip8(acc[p][1]), clip8(acc[p][2])};
    if (CH == 4) {
      const uint32_t al = clip8(acc[p][CH - 1]);
      if (al != 0u && al != 255u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { const uint32_t u = 255u * c[k] / al; c[k] = u > 255u ? 255u : u; }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) col[k][p] = color_chain(c[k]);
  }
  const long long plane = (long long)Ho * Wo;
  const long long out0 = (long long)y * Wo + xq;
  if (vec) {                                                                     // Wo % 4 == 0, 16-B aligned planes: whole quad
    *reinterpret_cast<float4*>(depth_out + out0) = make_float4(dep[0], dep[1], dep[2], dep[3]);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      *reinterpret_cast<float4*>(color_out + k * plane + out0) = make_float4(col[k][0], col[k][1], col[k][2], col[k][3]);
  } else {
    for (int p = 0; p < n; ++p) {
      depth_out[out0 + p] = dep[p];
#pragma unroll
      for (int k = 0; k < 3; ++k) color_out[k * plane + out0 + p] = col[k][p];
    }
  }
}

}  // namespace rtgs_ingest

extern "C" {

int rtgs_ingest_rgbd(const uint16_t* depth_raw, const uint8_t* color_raw, int32_t Hd, int32_t Wd, int32_t channels, int32_t crop,
                     float depth_scale, float* depth_out, float* color_out, void* stream) {
  using namespace rtgs_ingest;
  if (!depth_raw || !color_raw || !depth_out || !color_out) return -1;
  if (Hd <= 0 || Wd <= 0 || crop < 0 || (channels != 3 && channels != 4)) return -1;
  if (!(depth_scale > 0.0f)) return -1;
  const int H = Hd - 2 * crop, W = Wd - 2 * crop;
  if (H <= 0 || W <= 0) return -1;
  if ((long long)Hd * Wd * channels > 0x7fffffffLL) return -1;
  const long long nq = (long long)H * ((W + 3) / 4);
  const auto a16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
  const int aligned = (Wd % 4 == 0 && crop % 4 == 0 && W % 4 == 0 && a16(depth_raw) && a16(color_raw) && a16(depth_out) &&
                       a16(color_out)) ? 1 : 0;
  const int blocks = (int)((nq + NT - 1) / NT < MAX_BLOCKS ? (nq + NT - 1) / NT : MAX_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  if (channels == 4)
    hipLaunchKernelGGL(ingest_kernel<4>, dim3(blocks), dim3(NT), 0, st, depth_raw, color_raw, Wd, crop, H, W, depth_scale,
                       aligned, depth_out, color_out);
  else
    hipLaunchKernelGGL(ingest_kernel<3>, dim3(blocks), dim3(NT), 0, st, depth_raw, color_raw, Wd, crop, H, W, depth_scale,
                       aligned, depth_out, color_out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rtgs_ingest_rgbd_resized(const uint16_t* depth_raw, const uint8_t* color_raw, int32_t Hd, int32_t Wd, int32_t channels,
                             int32_t crop, float depth_scale, int32_t Ho, int32_t Wo, const int32_t* tables, int64_t tables_len,
                             int32_t x_ksize, int32_t y_ksize, float* depth_out, float* color_out, void* stream) {
  using namespace rtgs_ingest;
  if (!depth_raw || !color_raw || !depth_out || !color_out || !tables) return -1;
  if (Hd <= 0 || Wd <= 0 || crop < 0 || (channels != 3 && channels != 4)) return -1;
  if (!(depth_scale > 0.0f)) return -1;
  const int Hc = Hd - 2 * crop, Wc = Wd - 2 * crop;
  if (Hc <= 0 || Wc <= 0 || Ho <= 0 || Wo <= 0 || x_ksize <= 0 || y_ksize <= 0) return -1;
  if ((long long)Hd * Wd * channels > 0x7fffffffLL || (long long)Ho * Wo > 0x7fffffffLL) return -1;
  if (tables_len != 3LL * Wo + 3LL * Ho + (long long)Wo * x_ksize + (long long)Ho * y_ksize) return -1;
  // the source rows a tile of th output rows needs: window starts advance by at most ceil((th - 1) Hc / Ho) over the
  // tile, the last window adds y_ksize
  int th = RS_TH, R = 0;
  for (;; th >>= 1) {
    const long long step = ((long long)(th - 1) * Hc + Ho - 1) / Ho;
    const long long need = step + y_ksize + 1;
    if (need * RS_TW * 4 + (long long)th * y_ksize * 4 <= RS_LDS_MAX) { R = (int)need; break; }
    if (th == 1) return -1;                                   // one output row's window does not fit the LDS
  }
  // a small output gives few tiles, and a tile's time is a chain of load latencies: flatter tiles until every CU has one
  const long long gx = ((long long)Wo + RS_TW - 1) / RS_TW;
  while (th > 2 && gx * (((long long)Ho + th - 1) / th) < RS_MIN_TILES) {
    th >>= 1;
    R = (int)(((long long)(th - 1) * Hc + Ho - 1) / Ho) + y_ksize + 1;          // fewer rows than the taller tile: it fits
  }
  const long long gy = ((long long)Ho + th - 1) / th;
  if (gy > 65535 || gx > 0x7fffffffLL) return -1;
  const auto a16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
  const int vec = (Wo % 4 == 0 && a16(depth_out) && a16(color_out)) ? 1 : 0;
  const size_t lds = (size_t)R * RS_TW * 4 + (size_t)th * y_ksize * 4;        // staged rows + the tile's vertical coefficients
  hipStream_t st = (hipStream_t)stream;
  if (channels == 4)
    hipLaunchKernelGGL(ingest_resized_kernel<4>, dim3((unsigned)gx, (unsigned)gy), dim3(NT), lds, st, depth_raw, color_raw, Wd, crop,
                       Hc, Wc, Ho, Wo, depth_scale, tables, x_ksize, y_ksize, th, R, vec, depth_out, color_out);
  else
    hipLaunchKernelGGL(ingest_resized_kernel<3>, dim3((unsigned)gx, (unsigned)gy), dim3(NT), lds, st, depth_raw, color_raw, Wd, crop,
                       Hc, Wc, Ho, Wo, depth_scale, tables, x_ksize, y_ksize, th, R, vec, depth_out, color_out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
