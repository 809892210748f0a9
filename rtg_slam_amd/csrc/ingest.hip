// gfx950 kernel + C ABI of the frame ingest (include/rtgs_slam.h, "frame ingest"): the raw bytes of one decoded RGB-D frame
// (u16 depth [Hd,Wd], u8 colour [Hd,Wd,3|4]) -> the cropped float32 maps the SLAM loop consumes (depth [H,W] in metres,
// colour [3,H,W] in 0..1), H = Hd - 2 crop, W = Wd - 2 crop.
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

}  // extern "C"
