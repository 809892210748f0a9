// Host-side launch functions of the rasterizer's kernels: defined in raster_fwd.hip, raster_bwd.hip, raster_bwd_entry.hip
// and raster_bin.hip, called from raster_api.hip.  This is the ONE declaration of each: the four defining files include it
// too, so a definition that drifts from its prototype no longer matches it and the link (-Wl,--no-undefined) stops on
// the caller's symbol.  Default arguments live here and nowhere else.
#pragma once
#include "raster_common.h"

namespace rtgs {

// ---- raster_fwd.hip
void set_fwd_stamps(void* dev);
void launch_mask_sat(const int32_t* mask, int gx, int gy, int32_t* sat, hipStream_t st);
void launch_preprocess_fwd(const RasterParams& p, const float* means, const float* opac, const float* shs, const float* scales,
                           const float* rots, const float* normal_w, const int32_t* sat, Splat* splats, uint32_t* tiles_touched,
                           int32_t* radii, uint8_t* clamped, int32_t* out_radii, uint32_t* zero_words, int zero_n, uint8_t* zbin,
                           hipStream_t st);
void launch_preprocess_cull(const RasterParams& p, const float* means, const float* scales, const float* rots,
                            uint32_t* tiles_touched, int32_t* radii, int32_t* out_radii, uint32_t* zero_words, int zero_n,
                            uint8_t* zbin, float2* uv, uint32_t* hist_words, hipStream_t st);
void launch_preprocess_shade(const RasterParams& p, const float* means, const float* opac, const float* shs, const float* scales,
                             const float* rots, const float* normal_w, Splat* splats, int32_t* radii, uint8_t* clamped, float2* uv,
                             SliceList list, SliceSel sel, size_t max_items, hipStream_t st,
                             RowBands rb = RowBands{nullptr, nullptr, 0u});
void launch_recull_rows(const RasterParams& p, const float* means, const float* scales, const float* rots, uint32_t* tiles_touched,
                        int32_t* radii, int32_t* out_radii, uint32_t* zero_words, int zero_n, uint8_t* zbin, float2* uv,
                        uint32_t* hist, unsigned long long* cover, uint8_t* marks, const float* view_copy, int fail_idx,
                        BwdInfoInit bi, hipStream_t st);
void launch_cull_check(int P, const uint32_t* tt_a, const uint32_t* tt_b, const int32_t* rad_a, const int32_t* rad_b,
                       const int32_t* orad_a, const int32_t* orad_b, const uint8_t* zb_a, const uint8_t* zb_b, const float2* uv_a,
                       const float2* uv_b, const uint32_t* hist_a, const uint32_t* hist_b, const uint32_t* skip,
                       unsigned long long* mismatches, hipStream_t st);
void launch_emit_keys(const RasterParams& p, const Splat* splats, const int32_t* radii, const uint32_t* offsets,
                      const int32_t* mask, uint64_t* keys, uint32_t* vals, hipStream_t st);
void launch_tile_ranges(int64_t R, const uint64_t* keys, uint2* ranges, hipStream_t st);
void launch_slice_publish(int ntiles, const int32_t* user_mask, const int32_t* mask2, const uint32_t* r1, uint32_t* ctr,
                          uint32_t* host, uint32_t seq, uint32_t* spec_fail, hipStream_t st, const uint32_t* seg_count = nullptr);
void launch_blend_fwd(const RasterParams& p, const uint2* ranges, const uint32_t* point_list, const Splat* splats, float* out_color,
                      float* out_depth, int32_t* out_cidx, int32_t* out_didx, float* out_cw, float* out_dw, float* out_T,
                      uint32_t* n_contrib, unsigned long long* counters, SlicePass sp, uint32_t* tile_mode, uint32_t* depth_pos,
                      uint32_t* tile_last, int walk, uint32_t* aux_zero, TileCache tc, uint32_t seg, hipStream_t st,
                      FusedSort fs = FusedSort{nullptr, nullptr, nullptr, nullptr, nullptr},
                      TileGather tg = TileGather{nullptr, nullptr, 0u, nullptr, nullptr, nullptr});
bool blend_fwd_fuses_sort();
bool blend_fwd_gathers();

// ---- raster_bwd.hip
void launch_blend_bwd(const RasterParams& p, const uint2* ranges, const uint32_t* point_list, const Splat* splats,
                      const float* out_color, const float* final_T, const uint32_t* n_contrib, const int32_t* depth_index,
                      const float* dL_dcolor, const float* dL_ddepth, const uint32_t* gbase, uint32_t* slot_count,
                      const BwdInfo* info, SplatGrad* grads, uint8_t* touched, const uint32_t* tile_mode, int which, uint32_t t0,
                      uint32_t tn, hipStream_t st);
void launch_grad_reduce(int P, const uint8_t* touched, const uint32_t* gbase, uint32_t* count, const BwdInfo* info,
                        SplatGrad* grads, const uint32_t* spec_fail, hipStream_t st);
void launch_preprocess_bwd(const RasterParams& p, const float* means, const float* opac, const float* shs, const float* scales,
                           const float* rots, const float* normal_w, const int32_t* radii, const uint8_t* clamped,
                           SplatGrad* grads, uint8_t* touched, uint8_t* row_state, float* d_means, float* d_opac, float* d_shs,
                           float* d_scales, float* d_rots, float* d_normal, hipStream_t st);

// ---- raster_bwd_entry.hip
void set_bwd_debug(int bits);
void set_bwd_stamps(void* dev);
void launch_blend_bwd_entry(const RasterParams& p, const uint2* ranges, const uint32_t* point_list, const Splat* splats,
                            const float* out_color, const uint32_t* n_contrib, const int32_t* depth_index,
                            const uint32_t* depth_pos, const uint32_t* tile_last, const float* dL_dcolor, const float* dL_ddepth,
                            const uint32_t* gbase, uint32_t* slot_count, const BwdInfo* info, SplatGrad* grads, uint8_t* touched,
                            const uint32_t* tile_mode, uint32_t t0, uint32_t tn, TileCache tc, uint32_t pre, hipStream_t st,
                            const LossSigns* signs = nullptr);

// ---- raster_bin.hip
size_t bin_lds_limit_tiles();
int bin_sort_capacity();
size_t bin_block_counts_bytes(int P, int ntiles);
size_t bin_slice_block_counts_bytes(int P, size_t max_list, int ntiles);
size_t bin_list_block_counts_bytes(int P, int ntiles);
void launch_slice_hist(int P, const uint8_t* zbin, const uint32_t* rect_area, const int32_t* radii, uint32_t* hist,
                       unsigned long long* cover, hipStream_t st, BwdInfoInit bi = BwdInfoInit{nullptr, nullptr, 0u, 0u});
void launch_slice_compact(int P, SliceSel sel, uint32_t* ids, uint32_t* n_list, const uint32_t* rect_area, uint32_t* gbase,
                          uint32_t* slot_cursor, uint32_t* host, uint32_t seq, uint32_t* fail_if_taken, hipStream_t st);
void launch_visible_compact(int P, const uint8_t* zbin, uint32_t* ids, uint32_t* n_list, const uint32_t* rect_area,
                            uint32_t* gbase, uint32_t* slot_cursor, const uint32_t* spec_fail, hipStream_t st,
                            const SliceSel* decide = nullptr, int32_t* cut_out = nullptr, uint32_t* fail_if_taken = nullptr);
int launch_bin_count(const RasterParams& p, const Splat* splats, const int32_t* radii, const int32_t* mask, uint32_t* tile_count,
                     uint16_t* block_counts, SliceSel sel, SliceList list, size_t max_items, hipStream_t st);
void launch_bin_tilescan(int ntiles, const uint32_t* tile_count, uint2* ranges, uint32_t* cursor, uint32_t* info,
                         uint32_t* info_host, const uint32_t* extra_src, const uint32_t* extra_src2, const uint32_t* slot_a,
                         const uint32_t* slot_b, uint32_t seq, SpecCaps caps, hipStream_t st);
void launch_bin_scatter(const RasterParams& p, const Splat* splats, const int32_t* radii, const int32_t* mask,
                        const uint16_t* block_counts, uint32_t* cursor, unsigned long long* bucket, SliceSel sel, SliceList list,
                        size_t max_items, hipStream_t st);
void launch_bin_place(const RasterParams& p, const Splat* splats, const int32_t* radii, const int32_t* mask, uint32_t* seg_count,
                      unsigned long long* bucket, uint32_t seg, uint32_t* fail, SliceSel sel, SliceList list, size_t max_items,
                      hipStream_t st);
void launch_bin_tilesort(int ntiles, uint32_t longest, const uint2* ranges, const unsigned long long* bucket, uint32_t* point_list,
                         const uint32_t* spec_fail, hipStream_t st, const uint32_t* seg_count = nullptr, uint32_t seg = 0,
                         uint2* ranges_out = nullptr, const BinFinish* finish = nullptr);
void launch_bin_tilesort_long(int ntiles, const uint2* ranges, const unsigned long long* bucket, uint32_t* point_list,
                              const uint32_t* spec_fail, hipStream_t st, const uint32_t* seg_count, uint32_t seg);

}  // namespace rtgs
