/*
 * rtgs_slam.h - C ABI of the callers and data producers either side of RTG-SLAM's hot path (R9, f-1, f-3),
 * MI355X (gfx950) build.  Same conventions as rtgs_raster.h: device pointers, dense row-major float32 / int32 / uint8,
 * inputs borrowed, enqueued on `stream` (hipStream_t as void*), 0 = success / negative = error.
 *
 * What each entry point replaces in the reference:
 *   tile-mask producers      SLAM/utils.py:681-734 (pixelmask2tilemask, transmission2tilemask, colorerror2tilemask)
 *                            and the render-range step of mapper.py:471-508
 *   rtgs_knn3                simple_knn._C.distCUDA2 (un-vendored CUDA submodule; call site gaussian_pointcloud.py:376)
 *   rtgs_knn3_query          pytorch3d.ops.knn_points as Mapping.temp_points_filter uses it (mapper.py:803-827), and the
 *                            new-point rows of update_geometry's distCUDA2 (gaussian_pointcloud.py:366-381)
 *   rtgs_accumulate_error    cuda_utils._C.accumulate_gaussian_error (un-vendored; call site mapper.py:541-565)
 *   frame preprocessing      tracker.py:97-159 -> SLAM/utils.py:65-139 (vertex / normal / confidence maps),
 *                            SLAM/utils.py:550-589 (bilateral filter), SLAM/utils.py:141-183 (sample_pixels' mask)
 *   rtgs_gather_rows3        the normal-map gather of Renderer.render, SLAM/render.py:130-133
 *   rtgs_eval_*              SLAM/eval.py's picture metrics (utils/loss_utils.py psnr / l1_loss, pytorch_msssim.ms_ssim)
 *                            and the nearest-neighbour reduction of eval_pcd (scipy cKDTree queries: rtgs_knn3_query_built)
 *   rtgs_ingest_rgbd         the pixel arithmetic between the dataset files and the tracker: readCameras' depth scaling
 *                            (scene/dataset_readers.py:848-932), PILtoTorch (utils/general_utils.py:43-49) and map_preprocess's
 *                            * 255 (SLAM/multiprocess/tracker.py:97-101)
 *   rtgs_ingest_rgbd_resized the same with loadCam's resize in between (utils/camera_utils.py:22-74: PIL BILINEAR on the u8
 *                            colour, PIL NEAREST on the float depth), for resolution_scales other than 1
 *   rtgs_densify_discs       GaussianPointCloud.densify (SLAM/gaussian_pointcloud.py:53-116), the points slam.py:146-150
 *                            writes to save_model/pcd_densify.ply when the config sets pcd_densify
 */
#ifndef RTGS_SLAM_H
#define RTGS_SLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- tile masks (16 x 16 tiles unless `stride` says otherwise; the grid is ceil(H/stride) x ceil(W/stride), pixels
 *      beyond the image count as 0 exactly as the reference's zero padding) -------------------------------------- */

/* Per-tile SUM of a pixel map: src_kind 0 = uint8 mask (non-zero = 1), 1 = float32.  tile_sum[gy*gx] float32. */
int rtgs_tile_sum(const void* src, int32_t src_kind, int32_t H, int32_t W, int32_t stride, float* tile_sum, void* stream);

/* transmission2tilemask: tile on iff mean(mask) > ratio, i.e. sum > ratio * stride^2 (mask sums are exact integers). */
int rtgs_transmission2tilemask(const uint8_t* pixelmask, int32_t H, int32_t W, int32_t stride, float ratio,
                               int32_t* tile_mask, float* tile_sum_scratch, void* stream);
/* pixelmask2tilemask: tile on iff any pixel is. */
int rtgs_pixelmask2tilemask(const uint8_t* pixelmask, int32_t H, int32_t W, int32_t stride, int32_t* tile_mask,
                            float* tile_sum_scratch, void* stream);
/* colorerror2tilemask: the k = (int)(tiles * top_ratio) tiles with the largest mean error are on (ties at the k-th value:
 * lower tile index first).  Any number of tiles.  The reference computes int(numel * top_ratio) in double
 * (SLAM/utils.py:708-734); top_ratio crosses this ABI as float32, where e.g. 0.7 is 0.69999999 and k can come out one
 * short - a binding that holds the ratio in double computes k itself and calls the _k form (the Python host does). */
int rtgs_colorerror2tilemask(const float* color_error, int32_t H, int32_t W, int32_t stride, float top_ratio,
                             int32_t* tile_mask, float* tile_sum_scratch, void* stream);
int rtgs_colorerror2tilemask_k(const float* color_error, int32_t H, int32_t W, int32_t stride, int32_t top_k,
                               int32_t* tile_mask, float* tile_sum_scratch, void* stream);
/* The render-range step of mapper.py:471-508 in one call, straight from the rasterizer's T_map:
 *   render_mask = (T_map != 1)  [uint8, H*W],  tile_mask = transmission2tilemask(render_mask, 16, ratio),
 *   *count_out = number of set pixels (device uint32; render_ratio = count / pixels). */
int rtgs_render_range(const float* T_map, int32_t H, int32_t W, float ratio, uint8_t* render_mask, int32_t* tile_mask,
                      uint32_t* count_out, float* tile_sum_scratch, void* stream);

/* ---- simple_knn.distCUDA2 ------------------------------------------------------------------------------------- */
/* For each of the N points (float32 [N,3]): its three nearest OTHER points.  mean_dist2[N] = mean of the three squared
 * distances (d^2 = dx*dx + dy*dy + dz*dz in float32), idx[N,3] int32 ascending by distance, dist2[N,3] (may be NULL).
 * Exact (Morton order + bounding-box pruning, no approximation).  Fewer than three other points: FLT_MAX / -1.
 * scratch: rtgs_knn3_scratch_bytes(N) bytes. */
size_t rtgs_knn3_scratch_bytes(int32_t N);
int rtgs_knn3(const float* points, int32_t N, float* mean_dist2, int32_t* idx, float* dist2, void* scratch, void* stream);
/* Cross-set form: for each of the Nq QUERY points its three nearest REFERENCE points (idx[Nq,3] into ref_points, ascending
 * by distance; dist2[Nq,3], may be NULL; fewer than three references: -1 / FLT_MAX).  Exact, same search structure (built
 * over the references; queries are seeded by a binary search of their Morton code).  What it replaces in the reference:
 * pytorch3d.ops.knn_points(temp_xyz, exist_xyz, K=3) in Mapping.temp_points_filter (mapper.py:803-827), and - with
 * self_offset >= 0: query i IS reference self_offset + i and does not find itself - the `knn_indices[:points_num]` rows
 * of distCUDA2(total_xyz) in GaussianPointCloud.update_geometry (gaussian_pointcloud.py:366-381), which needs the
 * neighbours of the NEW points only.  self_offset < 0: the sets are unrelated.  ref_box6 (device float[6] = lo xyz, hi xyz;
 * NULL = none): references outside the OPEN box are ignored - bbox_filter (SLAM/utils.py:737-744), which both call sites
 * apply to the existing points before the search, without a compaction.  The queries are visited in Morton order (sorted
 * inside the call) so that the lanes of a wave open the same boxes.  scratch: rtgs_knn3_query_scratch_bytes(Nr, Nq). */
size_t rtgs_knn3_query_scratch_bytes(int32_t Nr, int32_t Nq);
int rtgs_knn3_query(const float* ref_points, int32_t Nr, const float* query_points, int32_t Nq, int32_t self_offset,
                    const float* ref_box6, int32_t* idx, float* dist2, void* scratch, void* stream);
/* The same search split by what changes between frames (round 6; Mapping.temp_to_optimize, i.e. update_geometry's neighbour
 * search over cat(new points, every existing Gaussian), gaussian_pointcloud.py:366-381).  build_ref leaves the search structure
 * of Nr >= 1 reference points in `built` (rtgs_knn3_built_bytes(Nr) bytes; it holds a COPY of the points: rebuild when they
 * change); query_built answers rtgs_knn3_query(self_offset = -1) against it (query_scratch: rtgs_knn3_query_built_scratch_bytes(Nq)).
 * dynamic_merge: for every query i its three nearest among (a) the three stable neighbours handed in (dist2_stable / idx_stable
 * [Nq,3], idx = stable row or -1), (b) the OTHER queries (query i is not its own neighbour) and (c) the Nu unstable points, the
 * last two compared directly; references outside the open box ref_box6 are ignored as above.  Result indices address
 * cat(queries, existing rows): query j -> j, stable row r -> Nq + r, unstable point u -> Nq + n_stable + u.  Same float32
 * distance expression as rtgs_knn3_query: the result equals the one-structure search up to the order of equidistant points. */
size_t rtgs_knn3_built_bytes(int32_t Nr);
size_t rtgs_knn3_query_built_scratch_bytes(int32_t Nq);
int rtgs_knn3_build_ref(const float* ref_points, int32_t Nr, void* built, void* stream);
int rtgs_knn3_query_built(const void* built, int32_t Nr, const float* query_points, int32_t Nq, const float* ref_box6, int32_t* idx,
                          float* dist2, void* query_scratch, void* stream);
int rtgs_knn3_dynamic_merge(const float* query_points, int32_t Nq, const float* unstable_points, int32_t Nu, int32_t n_stable,
                            const float* dist2_stable, const int32_t* idx_stable, const float* ref_box6, int32_t* idx, float* dist2,
                            void* stream);

/* ---- cuda_utils.accumulate_gaussian_error --------------------------------------------------------------------- */
/* FROZEN semantics (the CUDA source is absent; mapper.py:541-571 is the evidence): colour error goes to the Gaussian in
 * color_index, depth and normal error to the Gaussian in depth_index (-1 = nobody).  Outputs [P]: mean (mean != 0) or
 * sum of each error over the attributed pixels (0 where none), and outlier_count = attributed pixels over threshold.
 * scratch: 2 * P floats (pixel counts). */
int rtgs_accumulate_error(int32_t H, int32_t W, int32_t P, const float* color_err, const float* depth_err,
                          const float* normal_err, const int32_t* color_index, const int32_t* depth_index, float thr_c,
                          float thr_d, float thr_n, int32_t mean, float* g_color, float* g_depth, float* g_normal,
                          int32_t* outlier_count, float* scratch, void* stream);

/* ---- frame preprocessing --------------------------------------------------------------------------------------- */
/* bilateralFilter_torch(depth, radius, sigma_color, sigma_space) - SLAM/utils.py:550-589. */
int rtgs_bilateral_filter(const float* depth, int32_t H, int32_t W, int32_t radius, float sigma_color, float sigma_space,
                          float* out, void* stream);
/* The map part of Tracker.map_preprocess (tracker.py:114-131) after the optional filter: range mask, vertex / normal /
 * confidence maps, invalid-confidence mask zeroing all four.  K: device float[9].  Outputs: depth_out[H,W],
 * vertex_out[H,W,3], normal_out[H,W,3], conf_out[H,W], bad_out[H,W] uint8.  scratch: H*W*3 floats + 16 bytes. */
size_t rtgs_frame_preprocess_scratch_bytes(int32_t H, int32_t W);
int rtgs_frame_preprocess(const float* depth_in, int32_t H, int32_t W, const float* K, float min_depth, float max_depth,
                          float invalid_confidence_thresh, float* depth_out, float* vertex_out, float* normal_out,
                          float* conf_out, uint8_t* bad_out, void* scratch, void* stream);
/* Candidate pixels of sample_pixels (SLAM/utils.py:141-183): select_mask (NULL = all) minus pixels whose normal sums to
 * exactly 0, compacted IN INDEX ORDER: indices_out[*count_out] int32 flat pixel indices.  scratch: rtgs_compact_scratch_bytes. */
size_t rtgs_compact_scratch_bytes(int32_t n);
int rtgs_sample_candidates(const float* normal_map, const uint8_t* select_mask, int32_t H, int32_t W, int32_t* indices_out,
                           int32_t* count_out, uint8_t* flags_scratch, void* scratch, void* stream);

/* ---- Renderer.render's normal map (SLAM/render.py:130-133) ----------------------------------------------------- */
/* ---- per-frame mask / error producers of the mapper ------------------------------------------------------------- */
/* Mapping.temp_points_init (mapper.py:728-775) in one pass: transmission_mask = T > thr_T & depth > 0; error_mask =
 * ((|depth - render_depth| > thr_depth & depth > 0 & depth_index > -1) | (mean_c |frame - render colour| > thr_color &
 * depth > 0 & T < thr_T)) & ~transmission_mask; counts2[0..1] = set pixels of the two (device uint32, zeroed here).  Maps
 * are [H,W] (colours [3,H,W]) float32 / int32; masks uint8. */
int rtgs_add_masks(const float* T_map, const float* depth, const float* render_depth, const float* render_color_chw,
                   const float* frame_color_chw, const int32_t* depth_index, int32_t H, int32_t W, float thr_transmission,
                   float thr_depth, float thr_color, uint8_t* transmission_mask, uint8_t* error_mask, uint32_t* counts2,
                   void* stream);
/* Mapping.error_gaussians_remove (mapper.py:527-540): depth_error = |depth - render_depth|, 0 where the render lies behind the
 * frame, the frame has no depth or the pixel has no depth owner; color_error = sum_c |frame - render colour|, 0 where the
 * frame has no depth.  The inputs of rtgs_accumulate_error. */
int rtgs_frame_errors(const float* depth, const float* render_depth, const float* render_color_chw, const float* frame_color_chw,
                      const int32_t* depth_index, int32_t H, int32_t W, float* color_error, float* depth_error, void* stream);
/* Two bookkeeping passes of the mapper as single kernels (round 6).
 * error_counters - Mapping.error_gaussians_remove's strikes (mapper.py:541-565): for the first nf (stable) rows,
 * depth_counter += (g_depth > depth_strike_thr), color_counter += (g_color > color_strike_thr) (the caller passes twice the add
 * thresholds); delete_mask = depth_counter >= limit, release_mask = color_counter >= limit and not deleted; counts2 = their sums.
 * delete_mask - Mapping.gaussians_delete (mapper.py:298-335) for a cloud of n rows with activated scales [n,3]: radius
 * (sum - min) / 2 > 10 x the cloud's mean radius, or (add_tick != NULL) time_now - add_tick > window; count1 = set entries.  One
 * workgroup: meant for the unstable cloud (a few thousand rows). */
int rtgs_error_counters(int32_t nf, const float* g_color, const float* g_depth, float color_strike_thr, float depth_strike_thr,
                        int32_t* depth_counter, int32_t* color_counter, int32_t limit, uint8_t* delete_mask, uint8_t* release_mask,
                        uint32_t* counts2, void* stream);
int rtgs_delete_mask(int32_t n, const float* scales, const int32_t* add_tick, int32_t time_now, int32_t window, uint8_t* mask,
                     uint32_t* count1, void* stream);

/* The new Gaussians of a frame (round 6): what Mapping._new_points and the tail of Mapping.temp_to_optimize (this package's
 * mapping.py; the reference: GaussianPointCloud.add_empty_points / update_geometry, gaussian_pointcloud.py:305-405, compute_rot
 * SLAM/utils.py:216-221, mapper.py:886-899) spell as ~80 tensor operations, as two kernels with the same float32 operations.
 * gather_new_points: pick int64[n] (pixel indices into the [H*W,3] maps) -> xyz, UNIT normal (v / (|v| + 1e-8)), colour, rotation
 * quaternion (w,x,y,z) turning z onto the normal (identity_rot != 0: (1,0,0,0), the reference's branch for xyz_factor = 1,1,1).
 * (A pass of exactly THREE points must not come here: the reference's torch.cross without a dim then crosses along the batch.)
 * new_rows: candidate i with its three nearest neighbours (dist2 / idx [n,3] of rtgs_knn3_query over cat(candidates, existing);
 * idx < n names a candidate - radius 1e-6 -, idx >= n the existing Gaussian idx - n with activated scales exist_scales[., 3],
 * -1 no neighbour) -> packed59[n,59] raw rows (xyz | SH dc from the colour | zeros | raw opacity | log(scale_factor * s * factor)
 * | rotation) of EVERY candidate and valid[n] = 0 where the candidate lies inside three radii of a neighbour. */
int rtgs_gather_new_points(const int64_t* pick, int32_t n, const float* vertex_map, const float* normal_map, const float* color_map,
                           int32_t identity_rot, float* xyz, float* normal, float* color, float* rots, void* stream);
/* draw_new_points: SLAM/utils.py:171's `randperm(n_cand)[:k]` and gather_new_points in one launch.  cand int32[n_cand] = the
 * pixels sample_pixels may draw from (rtgs_sample_candidates); output i takes cand[perm(i)], perm a keyed bijection of
 * [0, n_cand) (balanced Feistel network + cycle walking; `key` = a fresh 64-bit word per pass from the caller's seeded
 * generator), so the k outputs are distinct.  pick_out int32[k] (optional) receives the drawn pixel indices.  k <= n_cand.
 * Not for k == 3 either.  filter_keep: Mapping.temp_points_filter's decision (mapper.py:812-826) behind the neighbour query:
 * keep[i] = 0 iff for one of the three neighbours idx[i,.] >= 0: sqrt(dist2) < ratio * radius(scales[idx]) (radius = (sum -
 * min) / 2 of the activated scales, gaussian_pointcloud.py:515-519; ratio 0.6).  bbox_pad: out6 = [min - pad | max + pad] of
 * n >= 1 points, the neighbour query's box (SLAM/utils.py:737-744), one single-workgroup launch. */
int rtgs_draw_new_points(const int32_t* cand, int32_t n_cand, int32_t k, uint64_t key, const float* vertex_map, const float* normal_map,
                         const float* color_map, int32_t identity_rot, float* xyz, float* normal, float* color, float* rots,
                         int32_t* pick_out, void* stream);
int rtgs_filter_keep(int32_t n, const float* dist2, const int32_t* idx, const float* scales, float ratio, uint8_t* keep, void* stream);
int rtgs_bbox_pad(int32_t n, const float* xyz, float pad, float* out6, void* stream);
/* The two ordered compactions of Mapping.temp_to_optimize as one single-workgroup launch each (the tensor form: nonzero - five
 * launches - and a gather per array).  compact_points: the candidates with keep[i] != 0 (the filter's survivors, mapper.py:826),
 * in order, into out_* (capacity n rows each); count_out int32[1] = how many.  append_valid_rows: the rows of packed59 [n,59]
 * (rtgs_new_rows) with valid[i] != 0, in order, split into the map's parameter blocks at xyz_dst [.,3] / shs_dst [.,48] /
 * raw8_dst [.,8] (pointers to the first free row; the caller guarantees n free rows), and for each of the n_aux <= 8 side arrays
 * (4-byte elements, one per row; host array of device pointers to the first free row) the 32-bit pattern aux_fill_bits[k];
 * count_out = how many rows were appended. */
int rtgs_compact_points(int32_t n, const uint8_t* keep, const float* xyz, const float* color, const float* opacity_raw,
                        const float* rots, float* out_xyz, float* out_color, float* out_opacity_raw, float* out_rots,
                        int32_t* count_out, void* stream);
int rtgs_append_valid_rows(int32_t n, const uint8_t* valid, const float* rows59, float* xyz_dst, float* shs_dst, float* raw8_dst,
                           int32_t n_aux, void* const* aux_dst, const uint32_t* aux_fill_bits, int32_t* count_out, void* stream);
int rtgs_new_rows(int32_t n, const float* xyz, const float* color, const float* opacity_raw, const float* rots, const float* dist2,
                  const int32_t* idx, const float* exist_scales, float min_radius, float max_radius, float scale_factor,
                  float factor_x, float factor_y, float factor_z, float* packed59, uint8_t* valid, void* stream);

/* Mapping.temp_points_attach (mapper.py:830-883): attach_out[i] = 1 iff point i projects (w2c16 row-major 4x4, pinhole fx fy
 * cx cy, truncation like Camera.get_uv, scene/cameras.py:161-168) inside the image onto a pixel whose stable colour index
 * is >= 0 and lies within max_plane_dist of that Gaussian's plane (stable_xyz / stable_normal rows). */
int rtgs_attach_test(const float* points, int32_t n, const float* w2c16, float fx, float fy, float cx, float cy, int32_t H,
                     int32_t W, const int32_t* stable_color_index, const float* stable_xyz, const float* stable_normal,
                     float max_plane_dist, uint8_t* attach_out, void* stream);
/* transform_map (SLAM/utils.py:56-63; tracker.py:283-288 builds vertex_map_w / normal_map_w with it): out[i] = T[:3,:3] in[i] +
 * T[:3,3] for n 3-vectors; transform16 = device float[16], row-major 4x4 (pass get_rot(c2w) - zero translation - for normals). */
int rtgs_transform_map(const float* map3, int64_t n, const float* transform16, float* out3, void* stream);
/* out[3,n]: out[:, p] = rows[index[p]] (rows float32 [N,3]) where index[p] >= 0, zeros elsewhere - the reference's two
 * boolean-mask indexings (two device-to-host syncs per render) as one kernel.  scatter = its backward: grad_rows[index[p]] +=
 * g[:, p] (accumulates; caller zeroes). */
int rtgs_gather_rows3(const float* rows, const int32_t* index, int32_t n, float* out, void* stream);
int rtgs_scatter_rows3(const float* g, const int32_t* index, int32_t n, float* grad_rows, void* stream);

/* ---- evaluation (SLAM/eval.py: eval_picture :38-147, eval_pcd :149-223) -------------------------------------------
 * Bitwise reproducible run to run: per-workgroup partials in scratch, reduced in a fixed order in float64; no float atomics.
 *
 * rtgs_eval_picture: render / gt_color [3,H,W], depth [1,H,W], gt_depth [H,W] (metres), depth_index [1,H,W] int32 (-1 = no
 * Gaussian).  Writes out[RTGS_EVAL_PICTURE_OUT] float64 on the device:
 *   psnr       mean over R, G, B of 20 log10(1 / sqrt(mse_c)), mse_c = mean over the H W pixels (mse_c = 0 -> +inf);
 *   color_l1   mean |gt - render| over the 3 H W values;
 *   depth      gt depth outside the OPEN interval (min_depth, max_depth) counts as 0; a pixel is valid iff depth_index != -1
 *              and gt != 0; valid_ratio = valid / (H W), depth_l1 = mean |depth - gt| over the valid pixels (NaN if none);
 *   ms_ssim    pytorch_msssim.ms_ssim(data_range 1) when with_ms_ssim != 0, else NaN: 11-tap Gaussian (sigma 1.5), VALID,
 *              C1 = 0.01^2, C2 = 0.03^2, 5 levels, weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), relu(mean cs) on levels
 *              0-3 and relu(mean ssim) on level 4, product of powers per channel, mean over channels; 2 x 2 average pooling
 *              between levels with a leading zero on odd axes and divisor 4.  Needs min(H, W) > RTGS_EVAL_MS_SSIM_MIN_SIDE
 *              (-1 otherwise).  Per-level means of cs / ssim per channel are in the vector too.
 * scratch: rtgs_eval_picture_scratch_bytes(H, W) bytes.
 *
 * rtgs_eval_nn_stats: column 0 (the nearest neighbour) of dist2 [N,3] float32 as rtgs_knn3_query_built leaves it; k <=
 * RTGS_EVAL_MAX_THRESHOLDS thresholds (device float64).  out[0] = sum of sqrt(d2) in float64, out[1 + j] = number of points
 * with sqrt(d2) < thresholds[j].  scratch: rtgs_eval_nn_stats_scratch_bytes(N, k) bytes. */
#define RTGS_EVAL_MS_SSIM_MIN_SIDE 160
#define RTGS_EVAL_MAX_THRESHOLDS 16
#define RTGS_EVAL_OUT_PSNR 0
#define RTGS_EVAL_OUT_COLOR_L1 1
#define RTGS_EVAL_OUT_DEPTH_L1 2
#define RTGS_EVAL_OUT_VALID_RATIO 3
#define RTGS_EVAL_OUT_MS_SSIM 4
#define RTGS_EVAL_OUT_VALID_COUNT 5
#define RTGS_EVAL_OUT_MSE 6                 /* 3 values, R G B */
#define RTGS_EVAL_OUT_CS 9                  /* 15 values, [level][channel] */
#define RTGS_EVAL_OUT_SSIM 24               /* 15 values, [level][channel] */
#define RTGS_EVAL_PICTURE_OUT 39              /* every slot is written */
size_t rtgs_eval_picture_scratch_bytes(int32_t H, int32_t W);
int rtgs_eval_picture(const float* render, const float* gt_color, const float* depth, const float* gt_depth,
                      const int32_t* depth_index, int32_t H, int32_t W, float min_depth, float max_depth, int32_t with_ms_ssim,
                      void* scratch, double* out, void* stream);
size_t rtgs_eval_nn_stats_scratch_bytes(int32_t N, int32_t k);
int rtgs_eval_nn_stats(const float* dist2, int32_t N, const double* thresholds, int32_t k, void* scratch, double* out,
                       void* stream);

/* ---- frame ingest (scene/dataset_readers.py:848-932 -> utils/general_utils.py:43-49 -> tracker.py:97-101) ----------
 * One launch per frame: raw u16 depth [Hd,Wd] and u8 colour [Hd,Wd,channels] (channels 3 or 4; a 4th channel is dropped)
 * -> depth_out [H,W] float32 and color_out [3,H,W] float32, H = Hd - 2 crop, W = Wd - 2 crop (the [c:-c, c:-c] crop of
 * readCameras).  Per pixel, each step one correctly rounded float32 operation, bit-identical to the reference's chain:
 *   depth_out = ((f32(raw) / depth_scale) / 255) * 255;   color_out[k] = f32(colour[k]) / 255.
 * Returns -1 on a bad shape, channel count, crop or scale (depth_scale must be > 0). */
int rtgs_ingest_rgbd(const uint16_t* depth_raw, const uint8_t* color_raw, int32_t Hd, int32_t Wd, int32_t channels, int32_t crop,
                     float depth_scale, float* depth_out, float* color_out, void* stream);

/* The same frame resized to Ho x Wo after the crop, as loadCam (utils/camera_utils.py:22-74) resizes it with PIL, in the same
 * single launch and bit-identical to that chain:
 *   colour  Image.resize((Wo, Ho), BILINEAR) on the cropped u8 image, then / 255.  Pillow's 8-bit resampler in integers: a
 *           horizontal pass, then a vertical pass on the rounded u8 result of the first; per pass
 *           out = clip_0..255((2^21 + sum_j coeff[j] * src[start + j]) >> 22).  A 4-channel image is resampled as
 *           Image.resize resamples RGBA: premultiplied by alpha before, divided by the resampled alpha after.
 *   depth   Image.resize((Wo, Ho), NEAREST) on f32(raw) / depth_scale: the pick of one source pixel, then / 255 * 255.
 * `tables` (device, int32, tables_len values) holds what depends on (cropped size, output size) only, computed on the host in
 * float64 as Pillow computes it (rtg_slam_amd.datasets.resample_tables / nearest_indices), in this order:
 *   x_start[Wo] x_len[Wo] x_near[Wo] y_start[Ho] y_len[Ho] y_near[Ho] x_coeff[Wo * x_ksize] y_coeff[Ho * y_ksize]
 * with start / len the source window of an output column or row (within the CROPPED image), coeff its 22-bit fixed-point
 * weights (zero beyond len), near the source index of the nearest pick, x_ksize / y_ksize the longest window.  Any ratio,
 * enlarging included; an output size equal to the cropped size works but rtgs_ingest_rgbd is the path for it.  The
 * horizontally resampled rows a tile's vertical windows cover are staged in LDS (no intermediate image in global memory);
 * the tile height shrinks from 16 rows to 1 as the reduction factor grows (and to 2 for outputs of few tiles).  Returns -1
 * on what rtgs_ingest_rgbd rejects, on a non-positive output size or window length, on a tables_len that is not
 * 3 Wo + 3 Ho + Wo x_ksize + Ho y_ksize, and when the window of a single output row does not fit 64 KiB of LDS (y_ksize
 * above ~250); windows are never truncated.
 * Indices read from `tables` are clamped to the buffers they address. */
int rtgs_ingest_rgbd_resized(const uint16_t* depth_raw, const uint8_t* color_raw, int32_t Hd, int32_t Wd, int32_t channels,
                             int32_t crop, float depth_scale, int32_t Ho, int32_t Wo, const int32_t* tables, int64_t tables_len,
                             int32_t x_ksize, int32_t y_ksize, float* depth_out, float* color_out, void* stream);

/* ---- densification (SLAM/gaussian_pointcloud.py:53-116, with get_normal / get_plane :539-571) -----------------------
 * Rows [row_begin, row_end) of the stable cloud: xyz [*,3], the activated scales [*,3] (exp of the raw scaling) and the
 * normalised rotations [*,4] (r, x, y, z; build_rotation normalises them once more, as the reference does).  cos_theta /
 * sin_theta [circle_num]: cos and sin of the reference's theta, computed by the caller.  K = sigma * levels * circle_num
 * points per Gaussian, point k = s (levels circle_num) + l circle_num + c of row r written to
 * out[((r - row_begin) K + k) 6 + 0..5] = x y z nx ny nz as float64 (the record of the PLY file): Gaussian-major, 64-bit
 * offsets.  The float32 chain is in csrc/densify.hip; scale ties sort to the lower axis index.  out must be 16-B aligned.
 * Returns 0 without a launch when row_end == row_begin; -1 on a bad range, count or pointer, or
 * K > RTGS_DENSIFY_MAX_POINTS_PER_GAUSSIAN. */
#define RTGS_DENSIFY_MAX_POINTS_PER_GAUSSIAN 2048
int rtgs_densify_discs(const float* xyz, const float* scales, const float* rotations, int64_t row_begin, int64_t row_end,
                       const float* cos_theta, const float* sin_theta, int32_t sigma, int32_t levels, int32_t circle_num,
                       double* out, void* stream);

/* ---- meshing: TSDF fusion and marching tetrahedra (no counterpart in the reference; csrc/tsdf.hip) ----------------------
 * The volume is a dense axis-aligned grid: corner lo3_host (3 floats on the HOST), dims (nx, ny, nz), edge `voxel`, x fastest.
 * Planes, all float32 on the device: tsdf [nz][ny][nx], weight [nz][ny][nx], rgb [3][nz][ny][nx]; a fresh volume holds
 * tsdf = 1, weight = 0, rgb = 0.  Voxel (ix, iy, iz) has linear index (iz ny + iy) nx + ix.
 *
 * rtgs_tsdf_integrate fuses one frame: depth [H][W] in metres (<= 0 = hole), color [3][H][W], pinhole fx fy cx cy, and
 * w2c12_host = the 3 rows of the world-to-camera rotation, then the translation (12 floats on the HOST).  Per voxel, in
 * float32 and in this order:
 *    p_w = lo + ((float)idx + 0.5f) voxel per axis;  p_c = R p_w + t, a row as ((r0 x + r1 y) + r2 z) + t;  skip if z_c <= 0;
 *    u = fx x_c / z_c + cx, v likewise;  px = (int)floorf(u + 0.5f), py likewise;  skip outside the image;
 *    d = depth[py][px], skip if d <= 0;  sdf = d - z_c, skip if sdf < -trunc;  s = fminf(1, sdf / trunc);
 *    tsdf = (tsdf w + s) / (w + 1);  rgb[c] = (rgb[c] w + color[c][py][px]) / (w + 1);  w = fminf(w + 1, max_weight).
 * By default blocks of 64 x 8 x 1 voxels that lie behind the camera, beyond the frame's largest depth + trunc or outside the
 * frustum are skipped before any of their voxels is loaded; rtgs_tsdf_set_dense (rtgs_debug.h) selects the one-thread-per-
 * voxel form.  Both forms write identical planes.  scratch: rtgs_tsdf_scratch_bytes(H, W) bytes on the device, 16-B aligned (the
 * frame interleaved as r g b depth, and its largest depth).
 *
 * Extraction.  A cell (its lower-corner voxel) is meshed when all 8 corners have weight >= min_weight; a corner is inside
 * when tsdf < 0.  The cell is split into the 6 tetrahedra around its main diagonal.  rtgs_tsdf_count writes the number of
 * triangles of every cell to counts [nz ny nx] (0 for the last layer of every axis).  rtgs_tsdf_emit, given those counts, their
 * EXCLUSIVE scan `offsets` and their sum n_tri, writes the triangles in the order (cell, tetrahedron, triangle): for corner
 * k of triangle j, keys[3 j + k] = (linear index of the crossed edge's lower endpoint) 7 + (edge class: the direction bits
 * x = 1, y = 2, z = 4 of the edge, minus 1), positions / colors [3 j + k][3] = the crossing interpolated from the lower
 * endpoint a to the upper b, p = p_a + (p_b - p_a) (t_a / (t_a - t_b)).  Equal keys carry bit-identical positions and colours.
 * Triangles are wound so that the normal points towards positive tsdf.  Returns -1 on a bad argument or a grid of more than
 * RTGS_TSDF_MAX_VOXELS voxels. */
#define RTGS_TSDF_MAX_VOXELS 2147483647LL
size_t rtgs_tsdf_scratch_bytes(int32_t H, int32_t W);
int rtgs_tsdf_integrate(float* tsdf, float* weight, float* rgb, int32_t nx, int32_t ny, int32_t nz, const float* lo3_host,
                        float voxel, float trunc, float max_weight, const float* depth, const float* color, int32_t H, int32_t W,
                        float fx, float fy, float cx, float cy, const float* w2c12_host, void* scratch, void* stream);
int rtgs_tsdf_count(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float min_weight,
                    int32_t* counts, void* stream);
int rtgs_tsdf_emit(const float* tsdf, const float* weight, const float* rgb, int32_t nx, int32_t ny, int32_t nz,
                   const float* lo3_host, float voxel, float min_weight, const int32_t* counts, const int64_t* offsets,
                   int64_t n_tri, int64_t* keys, float* positions, float* colors, void* stream);

/* The sparse brick volume (rtgs_tsdf_sparse_*): the same virtual grid - lo, dims, voxel, centres, 64-bit linear index
 * (iz ny + iy) nx + ix - with planes only for the 8 x 8 x 8 bricks near an observed surface.  Brick (bx, by, bz) covers voxels
 * [8 bx, 8 bx + 8) per axis, cut at the grid; brick dims nb = ceil(n / 8); brick linear index (bz nby + by) nbx + bx.
 *   table  [nbz][nby][nbx] int32: the brick's slot, -1 without one (the caller fills a new table with -1)
 *   pool   [slot][plane: tsdf, weight, r, g, b][z][y][x] float32, RTGS_TSDF_BRICK_BYTES a brick, 16-B aligned
 *   coords [slot][3] int32: (bx, by, bz)
 * A brick without a slot reads as a fresh volume (tsdf 1, weight 0, rgb 0), in extraction too.  One frame is three calls:
 *   rtgs_tsdf_sparse_mark      packs the frame into scratch (rtgs_tsdf_scratch_bytes) and writes flags [nbz nby nbx] int32: 1 for
 *                              every brick without a slot that holds one of the 27 neighbours (ix + dx, iy + dy, iz + dz),
 *                              d in {-1, 0, 1}^3, inside the grid, of an IN-BAND voxel: one the dense rule above updates and
 *                              whose sdf / trunc < 1 in float32; 0 elsewhere.
 *   rtgs_tsdf_sparse_allocate  given flags, their EXCLUSIVE scan `offsets` in brick-linear order and their sum n_new, gives
 *                              flagged brick i the slot base + offsets[i] (base = bricks allocated so far, base + n_new <=
 *                              capacity, the pool's and coords' size in bricks), writes table and coords and makes the new
 *                              bricks fresh.  Slots are thus in ascending brick linear index within a frame.
 *   rtgs_tsdf_sparse_integrate applies the dense rule's float chain to every voxel of the n_bricks allocated bricks; scratch
 *                              must still hold the frame packed by rtgs_tsdf_sparse_mark with the same arguments.  Voxels of
 *                              bricks without a slot are not updated: what was seen before a brick's allocation is lost.
 * Hence a voxel of an allocated brick equals the dense volume's bit for bit unless the dense voxel was updated before the
 * brick was allocated; after one frame into a fresh volume every allocated voxel and the whole mesh equal the dense ones.
 * rtgs_tsdf_sparse_count / _emit are rtgs_tsdf_count / _emit over the allocated bricks: counts and offsets are
 * [n_bricks][8][8][8] (slot, then z, y, x of the cell's lower corner in the brick); keys use the virtual linear index;
 * triangles leave in slot order, and cells [n_tri] receives each triangle's virtual cell linear index so that a stable sort
 * on it restores the (cell, tetrahedron, triangle) order.  min_weight must be > 0.  rtgs_tsdf_sparse_to_dense writes the box
 * window6_host = (x0, x1, y0, y1, z0, z1) (HOST, voxels, half-open) as dense planes tsdf, weight [wz][wy][wx], rgb [3][wz][wy][wx].
 * Limits: every dim <= 2^24, nbx nby nbz and capacity <= RTGS_TSDF_SPARSE_MAX_BRICKS; nx ny nz only has to fit int64.
 * Returns -1 on a bad argument. */
#define RTGS_TSDF_SPARSE_MAX_BRICKS 2147483647LL
#define RTGS_TSDF_BRICK_BYTES 10240
int rtgs_tsdf_sparse_mark(const int32_t* table, int32_t* flags, int32_t nx, int32_t ny, int32_t nz, const float* lo3_host,
                          float voxel, float trunc, const float* depth, const float* color, int32_t H, int32_t W, float fx, float fy,
                          float cx, float cy, const float* w2c12_host, void* scratch, void* stream);
int rtgs_tsdf_sparse_allocate(int32_t* table, const int32_t* flags, const int64_t* offsets, int32_t nx, int32_t ny, int32_t nz,
                              int64_t base, int64_t n_new, int64_t capacity, int32_t* coords, float* pool, void* stream);
int rtgs_tsdf_sparse_integrate(float* pool, const int32_t* coords, int64_t n_bricks, int32_t nx, int32_t ny, int32_t nz,
                               const float* lo3_host, float voxel, float trunc, float max_weight, int32_t H, int32_t W, float fx,
                               float fy, float cx, float cy, const float* w2c12_host, const void* scratch, void* stream);
int rtgs_tsdf_sparse_count(const float* pool, const int32_t* coords, const int32_t* table, int64_t n_bricks, int32_t nx,
                           int32_t ny, int32_t nz, float min_weight, int32_t* counts, void* stream);
int rtgs_tsdf_sparse_emit(const float* pool, const int32_t* coords, const int32_t* table, int64_t n_bricks, int32_t nx, int32_t ny,
                          int32_t nz, const float* lo3_host, float voxel, float min_weight, const int32_t* counts,
                          const int64_t* offsets, int64_t n_tri, int64_t* cells, int64_t* keys, float* positions, float* colors,
                          void* stream);
int rtgs_tsdf_sparse_to_dense(const float* pool, const int32_t* table, int32_t nx, int32_t ny, int32_t nz, const int32_t* window6_host,
                              float* tsdf, float* weight, float* rgb, void* stream);

/* ---- mesh operations: normals, components, compaction, vertex clustering (no counterpart in the reference; csrc/mesh_ops.hip)
 * An indexed triangle mesh on the device: vertices [V][3] float32, faces [F][3] int32, colours [V][3] float32, as
 * rtgs_tsdf_emit's triangles are welded into, or as another of these operations leaves it.  The CALLER guarantees
 * 0 <= faces[i] < V; V, F <= RTGS_MESH_MAX_ELEMENTS.  Every result is unique and independent of thread order (no float atomics):
 * two runs are bit-equal, and tests/mesh_ops_reference.py restates each in numpy.  Scans and sorts are the caller's.
 *
 * rtgs_mesh_vertex_normals.  order [3 F] = the corner indices o = 3 f + k sorted STABLY by faces[o]; start [V + 1] = the first
 *   position of every vertex's run in it (start[V] = 3 F).  Face normal n = e1 x e2 with e1 = p1 - p0, e2 = p2 - p0, a component
 *   two rounded float32 products and a rounded difference (area-weighted); a vertex's sum starts at 0 and adds its corners'
 *   face normals in ascending o, every addition rounded; normals [V][3] = sum / l, l = sqrtf((x x + y y) + z z), when l > 0,
 *   else 0 0 0.
 * rtgs_mesh_component_labels.  labels [V] = the smallest vertex index joined to v through faces (two vertices of a face are
 *   joined); an unreferenced vertex labels itself.  parent [V] int32 is scratch (a lock-free union-find: a root is hooked
 *   under a smaller root by compare-and-swap, so every chain descends and every retry lowers an index - no unbounded loop).
 * rtgs_mesh_component_faces adds 1 to counts[labels[faces[f][0]]] for every face (counts [V], zeroed by the caller);
 *   rtgs_mesh_keep_faces then writes keep [F] = 1 where the face's component has at least min_faces faces, else 0.
 * rtgs_mesh_mark_vertices writes used[v] = 1 (used [V], zeroed by the caller) for the corners of every face with keep[f] != 0
 *   (keep may be NULL: every face).  rtgs_mesh_compact_vertices, given used and its EXCLUSIVE scan offsets, copies every used
 *   vertex and colour to row offsets[v], in order, and writes vmap [V] = the new index, -1 for a dropped vertex.
 *   rtgs_mesh_compact_faces copies face f with keep[f] != 0 to row offsets[f] (the EXCLUSIVE scan of keep; keep NULL: every face
 *   to its own row), its indices passed through vmap (NULL: unchanged).
 * rtgs_mesh_cluster_cells.  cells [V][3] = (int) floorf((p - origin) / cell) per axis in float32, origin3_host 3 floats on the
 *   HOST; err[0] (zeroed by the caller) is set to 1 when a coordinate is below origin or NaN, or its cell index is not below
 *   RTGS_MESH_MAX_CELLS.  rtgs_mesh_cluster_means, given the vertex indices `order` sorted STABLY by cell key and the S + 1 run
 *   starts, writes per run the mean position and colour: members added in float64 in that order, divided by the count in
 *   float64, rounded to float32.  rtgs_mesh_cluster_faces maps faces through cluster [V] (a vertex's run index), rotates each
 *   so that its smallest index comes first (winding kept) and writes valid [F] = 0 for a face with two corners in one run.
 *   rtgs_mesh_mark_first, given those faces and ids [n] = the valid faces sorted STABLY by their three indices, writes
 *   keep[ids[i]] = 1 for the first of every run of identical faces - the first in original order - and 0 for the others.
 * Return 0 (also, without a launch, for an empty mesh), -1 on a bad argument, -2 on a launch failure. */
#define RTGS_MESH_MAX_ELEMENTS 2147483647LL
#define RTGS_MESH_MAX_CELLS 2097152
int rtgs_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t V, int64_t F, const int64_t* order,
                             const int64_t* start, float* normals, void* stream);
int rtgs_mesh_component_labels(const int32_t* faces, int64_t F, int64_t V, int32_t* parent, int32_t* labels, void* stream);
int rtgs_mesh_component_faces(const int32_t* faces, int64_t F, const int32_t* labels, int32_t* counts, void* stream);
int rtgs_mesh_keep_faces(const int32_t* faces, int64_t F, const int32_t* labels, const int32_t* counts, int32_t min_faces,
                         int32_t* keep, void* stream);
int rtgs_mesh_mark_vertices(const int32_t* faces, int64_t F, const int32_t* keep, int32_t* used, void* stream);
int rtgs_mesh_compact_vertices(const float* vertices, const float* colors, int64_t V, const int32_t* used, const int64_t* offsets,
                               float* out_vertices, float* out_colors, int32_t* vmap, void* stream);
int rtgs_mesh_compact_faces(const int32_t* faces, int64_t F, const int32_t* keep, const int64_t* offsets, const int32_t* vmap,
                            int32_t* out_faces, void* stream);
int rtgs_mesh_cluster_cells(const float* vertices, int64_t V, const float* origin3_host, float cell, int32_t* cells, int32_t* err,
                            void* stream);
int rtgs_mesh_cluster_means(const float* vertices, const float* colors, const int64_t* order, const int64_t* start, int64_t S,
                            float* out_vertices, float* out_colors, void* stream);
int rtgs_mesh_cluster_faces(const int32_t* faces, int64_t F, const int32_t* cluster, int32_t* out_faces, int32_t* valid,
                            void* stream);
int rtgs_mesh_mark_first(const int32_t* faces, const int64_t* ids, int64_t n, int32_t* keep, void* stream);

/* ---- mesh decimation: parallel quadric-error half-edge collapse (no counterpart in the reference; csrc/mesh_decimate.hip).
 * The same mesh and the same guarantees as the mesh operations above.  A collapse u -> v removes vertex u and moves nothing;
 * the float work is float64, one rounded operation per step, in the order tests/mesh_decimate_reference.py writes out, and
 * the kernels match it bit for bit.  The caller (rtg_slam_amd/mesh_ops.py decimate) runs rounds on the CURRENT faces, with
 * `order` and `start` as for rtgs_mesh_vertex_normals; its sorts and scans sit between the calls.
 *
 * rtgs_mesh_decimate_quadrics, once.  quadrics [V][11] float64: per face in its stored corner order n = (pb - pa) x (pc - pa)
 *   (a component two products and a difference), l = sqrt((nx nx + ny ny) + nz nz); nothing unless l > 0; pl = (n / l,
 *   -(((nx/l) pax + (ny/l) pay) + (nz/l) paz)), w = l / 2; the record is w (pl_i pl_j) for the 10 pairs i <= j in row order,
 *   then w.  A vertex's quadric starts at 0 and adds its corners' records in ascending corner index.
 * rtgs_mesh_decimate_edge_keys.  keys [3 F] int64 = min V + max of the edges (a,b) (b,c) (c,a).  rtgs_mesh_decimate_locks,
 *   given the n distinct keys in ascending order and their counts, writes locked[x] = 1 (locked [V], zeroed by the caller)
 *   for both vertices of every edge whose count is not 2.
 * rtgs_mesh_decimate_propose.  Vertex u is removable when it is not locked and has RTGS_MESH_DECIMATE_MIN_VALENCE ..
 *   RTGS_MESH_DECIMATE_MAX_VALENCE faces.  A neighbour v is valid when (a) N(u) and N(v) share exactly 2 vertices, (b) every
 *   face (u, x, y) of u without v has ((px - pu) x (py - pu)) . ((px - pv) x (py - pv)) > 0, the dot (xx + yy) + zz, or p_v == p_u, and (d)
 *   with max_error > 0 (0: no bound), sqrt(cost / q[10]) <= max_error; (c) q = Q[u] + Q[v], cost = p_v^T q p_v as r_i =
 *   ((q_i0 x + q_i1 y) + q_i2 z) + q_i3, ((r0 x + r1 y) + r2 z) + r3, and 0 unless that is > 0.  proposal [V] = the valid v
 *   with the smallest (cost, v), -1 without one or for a vertex that is not removable; cost [V] float64 = its cost.
 * rtgs_mesh_decimate_claim.  ranked [>= P] int64 = the proposing vertices in rank order.  Participant r < P lowers claim[x]
 *   (claim [V] int32, filled with INT32_MAX by the caller) to r, by atomicMin, for every x of N[u] + N[v], the closed
 *   neighbourhoods.  rtgs_mesh_decimate_select then writes selected [P] = 1 where claim[x] == r for all of them, else 0: two
 *   selected collapses have disjoint N[u] + N[v].
 * rtgs_mesh_decimate_apply.  For every r < P with applied[r] != 0: remap[u] = v (remap [V], the identity before the first
 *   round) and Q[v] = Q[v] + Q[u].  rtgs_mesh_decimate_reindex writes keep [F] = 0 for a face two of whose corners are equal
 *   after remap, else 1; rtgs_mesh_compact_faces with vmap = remap then gives the next round's faces.
 * Return 0 (also, without a launch, for nothing to do), -1 on a bad argument (a null pointer that is needed, a count < 0 or
 * >= 2^31, a NaN max_error), -2 on a launch failure. */
#define RTGS_MESH_DECIMATE_MIN_VALENCE 4
#define RTGS_MESH_DECIMATE_MAX_VALENCE 32
#define RTGS_MESH_DECIMATE_MAX_ROUNDS 1000
int rtgs_mesh_decimate_quadrics(const float* vertices, const int32_t* faces, int64_t V, int64_t F, const int64_t* order,
                                const int64_t* start, double* quadrics, void* stream);
int rtgs_mesh_decimate_edge_keys(const int32_t* faces, int64_t F, int64_t V, int64_t* keys, void* stream);
int rtgs_mesh_decimate_locks(const int64_t* keys, const int64_t* counts, int64_t n, int64_t V, int32_t* locked, void* stream);
int rtgs_mesh_decimate_propose(const float* vertices, const int32_t* faces, int64_t V, int64_t F, const int64_t* order,
                               const int64_t* start, const int32_t* locked, const double* quadrics, double max_error,
                               int32_t* proposal, double* cost, void* stream);
int rtgs_mesh_decimate_claim(const int32_t* faces, const int64_t* order, const int64_t* start, const int64_t* ranked,
                             const int32_t* proposal, int64_t P, int32_t* claim, void* stream);
int rtgs_mesh_decimate_select(const int32_t* faces, const int64_t* order, const int64_t* start, const int64_t* ranked,
                              const int32_t* proposal, int64_t P, const int32_t* claim, int32_t* selected, void* stream);
int rtgs_mesh_decimate_apply(const int64_t* ranked, const int32_t* proposal, const int32_t* applied, int64_t P, int32_t* remap,
                             double* quadrics, void* stream);
int rtgs_mesh_decimate_reindex(const int32_t* faces, int64_t F, const int32_t* remap, int32_t* keep, void* stream);

/* ---- visibility: which points a depth frame saw, which faces that leaves (no counterpart in the reference;
 * csrc/visibility.hip).  tests/visibility_reference.py restates both in numpy; the kernels match it bit for bit.
 *
 * rtgs_visibility_add.  points [N][3] float32 in the frame w2c maps FROM; depth [H][W] float32 in metres; w2c12_host = the top
 *   three rows of the world-to-camera matrix, 12 floats on the HOST (passed to the kernel by value); views [N] int32, the
 *   caller's running counts.  Per point, float32, one correctly rounded operation per step:
 *     1  xc = ((m0 x + m1 y) + m2 z) + m3, yc and zc likewise from rows 1 and 2
 *     2  fail unless zc > 0
 *     3  u = fx xc / zc + cx,  v = fy yc / zc + cy
 *     4  pu = floorf(u + 0.5f),  pv = floorf(v + 0.5f)
 *     5  fail unless 0 <= pu < W and 0 <= pv < H
 *     6  d = depth[pv][pu]; fail unless d > 0 (a hole sees nothing)
 *     7  fail when zc - d > tolerance (the point is behind what the sensor measured)
 *     8  views[i] += 1
 *   Every comparison is false for NaN, so a NaN coordinate fails.  views[i] is read and written only in step 8, by the one
 *   thread that owns point i: no atomics.  tolerance >= 0.
 * rtgs_visibility_keep_faces.  keep [F] = 1 where all three corners of faces [F][3] (any_vertex != 0: at least one) have
 *   views >= min_views, else 0.  The CALLER guarantees 0 <= faces[i] < the length of views.
 * Return 0 (also, without a launch, for N == 0 / F == 0), -1 on a bad argument, -2 on a launch failure. */
int rtgs_visibility_add(const float* points, int64_t N, const float* depth, int32_t H, int32_t W, float fx, float fy, float cx,
                        float cy, const float* w2c12_host, float tolerance, int32_t* views, void* stream);
int rtgs_visibility_keep_faces(const int32_t* faces, int64_t F, const int32_t* views, int32_t min_views, int32_t any_vertex,
                               int32_t* keep, void* stream);

/* ---- mesh render: the depth map and the face map of an indexed triangle mesh at a pinhole pose (no counterpart in the
 * reference; csrc/mesh_render.hip).  tests/mesh_render_reference.py restates it in numpy; the kernels match it bit for bit.
 *
 * vertices [V][3] float32 in the frame w2c maps FROM; faces [F][3] int32, the CALLER guarantees 0 <= faces[i] < V;
 * w2c12_host = the top three rows of the world-to-camera matrix, 12 floats on the HOST; depth [H][W] float32 (0 where nothing
 * was hit) and face [H][W] int32 (-1 there).  Float32, one correctly rounded operation per step:
 *   per vertex  xc, yc, zc, u, v as steps 1 and 3 of rtgs_visibility_add, iz = 1 / zc; usable when zc > near (NaN fails)
 *   per face    dropped whole when a corner is not usable (NO clipping: a face across the near plane leaves a hole) or when a
 *               u or v is not finite.  x0 = max(ceil(min u), 0), x1 = min(floor(max u), W - 1), y0 and y1 likewise from v
 *               and H, all in float; skipped unless x0 <= x1 and y0 <= y1; integers only after that.  Pixel centres are the
 *               integer coordinates.
 *   edge p->q   E = (qu - pu)(py - pv) - (qv - pv)(px - pu), evaluated with the ends in lexicographic (u, v) order and negated
 *               when that reverses the edge; ends that project to one point drop the face.  w0 = E(b,c), w1 = E(c,a),
 *               w2 = E(a,b), area = (w0 + w1) + w2; covered when all w >= 0 and area > 0, or all w <= 0 and area < 0.
 *   depth       z = 1 / (((w0 iz_a + w1 iz_b) + w2 iz_c) / area), accepted when finite and > 0
 *   resolve     the pixel keeps the smallest key (bits(z) << 32) | face: the nearest surface, then the lowest face index.
 * One call is four launches on `stream` (clear, faces, large faces, resolve) with no host read.  A face whose box holds at
 * most small_max (>= 0) pixels is walked by one thread, a larger one by a wave, through a queue of F entries in the scratch; the
 * picture does not depend on small_max.  scratch: rtgs_mesh_render_scratch_bytes bytes (0 for sizes rtgs_mesh_render
 * refuses), the caller's, reusable by the next call, 8-byte aligned.  F == 0 gives the empty picture.
 * Return 0, -1 on a bad argument (F or H W >= 2^31, near <= 0 or NaN, small_max < 0, a null pointer that is needed), -2 on a
 * launch failure. */
size_t rtgs_mesh_render_scratch_bytes(int64_t V, int64_t F, int32_t H, int32_t W);
int rtgs_mesh_render(const float* vertices, int64_t V, const int32_t* faces, int64_t F, int32_t H, int32_t W, float fx, float fy,
                     float cx, float cy, const float* w2c12_host, float near, int32_t small_max, void* scratch, float* depth,
                     int32_t* face, void* stream);

/* The colour pass: a picture of the mesh from a face map rtgs_mesh_render made at this pose, coloured from the vertices or from
 * a texture atlas.  tests/mesh_shade_reference.py restates it in numpy; the kernel matches it bit for bit.
 *
 * vertices, faces, H, W, fx .. cy, w2c12_host, near as rtgs_mesh_render was given them; face_map [H][W] int32.  Exactly one
 * source: colors [V][3] float32 in 0..1, or uv [F][3][2] float32 (a face's three texture coordinates, x right and y down in
 * 0..1, as meshing.texture_mesh gives them) with texture [Ht][Wt][3] uint8; the other source's pointers are null.
 * background3_host: 3 floats on the HOST.  out [3][H][W] float32.  Float32, one correctly rounded operation per step, per pixel
 * (px, py) with f = face_map[py][px]:
 *   no face     f < 0, f >= F, or the face setup of rtgs_mesh_render fails for f at this view: the pixel gets the background
 *   weights     w0 = E(b,c), w1 = E(c,a), w2 = E(a,b) at ((float)px, (float)py), the values whose signs admitted the pixel;
 *               b0 = w0 iz_a, b1 = w1 iz_b, b2 = w2 iz_c, s = (b0 + b1) + b2, l_k = b_k / s (perspective-correct); an l_k that
 *               is not finite gives the background
 *   vertices    per channel c = (l0 c_a + l1 c_b) + l2 c_c, then fminf(fmaxf(c, 0), 1)
 *   texture     tu = (l0 u_a + l1 u_b) + l2 u_c, tv likewise; X = fminf(fmaxf(tu (float)Wt - 0.5, 0), (float)(Wt - 1)) (a NaN
 *               gives 0), ix = floorf(X), ix1 = min(ix + 1, Wt - 1), tx = X - ix; Y, iy, iy1, ty likewise with Ht; a texel is
 *               (float)byte / 255; top = c00 + tx (c10 - c00), bot = c01 + tx (c11 - c01), c = top + ty (bot - top)
 * One launch on `stream`, one thread per pixel, no host read, no scratch.  Any face map is safe to pass: nothing is read out of
 * bounds as long as 0 <= faces[i] < V.  F == 0 gives the background everywhere.
 * Return 0, -1 on a bad argument (a null pointer that is needed; no source or both; uv without texture or the reverse; Ht or Wt
 * < 1 or > RTGS_MESH_TEXTURE_MAX_SIDE; F or H W >= 2^31; near <= 0 or NaN), -2 on a launch failure. */
int rtgs_mesh_shade(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int32_t* face_map, int32_t H, int32_t W,
                    float fx, float fy, float cx, float cy, const float* w2c12_host, float near, const float* colors, const float* uv,
                    const uint8_t* texture, int32_t Ht, int32_t Wt, const float* background3_host, float* out, void* stream);

/* ---- mesh distance: the exact distance from a point to the nearest triangle of an indexed mesh, with that triangle's index (no
 * counterpart in the reference; csrc/mesh_distance.hip).  tests/mesh_distance_reference.py restates it in numpy as a brute
 * force over all faces; the kernels match it bit for bit, whatever the grid.
 *
 * vertices [V][3] float32, finite, |coordinate| <= 2^20; faces [F][3] int32, the CALLER guarantees 0 <= faces[i] < V; F >= 1.
 * The grid is the caller's: origin_host (3 floats on the HOST), cell > 0, dims_host (3 ints on the HOST, each in
 * 1..RTGS_MESH_DISTANCE_MAX_DIM, their product < 2^31), and vmax = the largest |coordinate| of the vertices.  The CALLER
 * guarantees that every vertex lies at least half a cell inside the grid's box.  Cell (x, y, z) has the index (z ny + y) nx + x.
 *   pair_d2(p, face)  float32, one correctly rounded operation per step: the minimum of the three edge values seg(p, s, e) - d = e - s,
 *                     w = p - s, t = clamp01(w.d / d.d) (0 when d.d is not > 0), q = w - t d, q.q; the ends ordered by vertex
 *                     index, lower first - and, when det = ab.ab ac.ac - (ab.ac)^2 > 0, of the interior value: s, t the
 *                     barycentrics by Cramer's rule, s clamped into [0, 1], t into [0, 1 - s], q = (w - s ab) - t ac, q.q.
 *                     u.v = (ux vx + uy vy) + uz vz; clamp01(NaN) = 0.
 *   result            d2[i] = the minimum of pair_d2 over ALL faces, face[i] = the lowest face index attaining it; a point with a
 *                     non-finite coordinate gives (+inf, -1).
 * rtgs_mesh_distance_count   counts [cells] int32, ZEROED by the caller, += 1 per face registered in the cell (every cell of the
 *   face's inflated box that its inflated plane crosses).  A box of more than large_max (>= 0) cells is walked by a wave
 *   through the queue in queue_scratch: rtgs_mesh_distance_queue_bytes(F) bytes whose first 16 the caller ZEROED, 4-byte aligned.
 * rtgs_mesh_distance_fill    after the caller's exclusive scan start [cells + 1] int32 of counts: entries [start[cells]] int32 are
 *   written through cursor [cells] int32, ZEROED by the caller; queue_scratch as count left it, same large_max.  The order of a
 *   cell's entries is not defined.
 * rtgs_mesh_distance_blocks  occupied uint8: first one flag per block of B^3 cells, [ceil(nx/B) ceil(ny/B) ceil(nz/B)] = [bz][by][bx],
 *   B = RTGS_MESH_DISTANCE_BLOCK, 1 where a cell of the block has an entry; then one flag per super block of S^3 blocks,
 *   [ceil(bz/S)][ceil(by/S)][ceil(bx/S)], S = RTGS_MESH_DISTANCE_SUPER, 1 where a block of it is occupied.
 * rtgs_mesh_distance_query   points [N][3] float32 (anywhere), order: NULL, or a permutation of 0..N-1 (int64) in which the threads
 *   take the points; d2 [N] float32 and face [N] int32 are written at the points' own rows.  One launch, no host read.
 * rtgs_mesh_distance_query_bounded  "the nearest face within max_d2, or nothing": row i is the row of rtgs_mesh_distance_query when
 *   its d2[i] <= max_d2 (float32; equality keeps the row, a NaN drops it) and (+inf, -1) otherwise, so also for a non-finite
 *   point.  max_d2 = +inf is the unbounded result, max_d2 = 0 keeps only exact zeros; max_d2 < 0 or NaN returns -1.  A kernel of
 *   its own: the walk starts under the bound, so a point far from every face ends after the first rings of super blocks.
 *   tests/mesh_distance_bounded_reference.py (nearest_within) is the definition.
 * rtgs_mesh_distance_keys    keys [N] int64: the point's cell, clamped into the grid, block-major (0 for a non-finite point).
 * rtgs_mesh_distance_normals normals [N][3] float32: n = (b - a) x (c - a) of face[i] as rtgs_mesh_vertex_normals forms it,
 *   divided by l = sqrt((x x + y y) + z z) when l > 0; (0, 0, 0) otherwise and for face[i] < 0.
 * Return 0 (also, without a launch, for N == 0), -1 on a bad argument, -2 on a launch failure. */
#define RTGS_MESH_DISTANCE_BLOCK 4
#define RTGS_MESH_DISTANCE_SUPER 4
#define RTGS_MESH_DISTANCE_MAX_DIM 65536
size_t rtgs_mesh_distance_queue_bytes(int64_t F);
int rtgs_mesh_distance_count(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const float* origin_host, float cell,
                             const int32_t* dims_host, float vmax, int32_t large_max, int32_t* counts, void* queue_scratch, void* stream);
int rtgs_mesh_distance_fill(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const float* origin_host, float cell,
                            const int32_t* dims_host, float vmax, int32_t large_max, const int32_t* start, int32_t* cursor, int32_t* entries,
                            void* queue_scratch, void* stream);
int rtgs_mesh_distance_blocks(const int32_t* start, const float* origin_host, float cell, const int32_t* dims_host, uint8_t* occupied,
                              void* stream);
int rtgs_mesh_distance_query(const float* points, int64_t N, const int64_t* order, const float* vertices, int64_t V, const int32_t* faces,
                             int64_t F, const float* origin_host, float cell, const int32_t* dims_host, float vmax, const int32_t* start,
                             const int32_t* entries, const uint8_t* occupied, float* d2, int32_t* face, void* stream);
int rtgs_mesh_distance_query_bounded(const float* points, int64_t N, const int64_t* order, const float* vertices, int64_t V,
                                     const int32_t* faces, int64_t F, const float* origin_host, float cell, const int32_t* dims_host, float vmax,
                                     const int32_t* start, const int32_t* entries, const uint8_t* occupied, float max_d2, float* d2,
                                     int32_t* face, void* stream);
int rtgs_mesh_distance_keys(const float* points, int64_t N, const float* origin_host, float cell, const int32_t* dims_host, int64_t* keys,
                            void* stream);
int rtgs_mesh_distance_normals(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int32_t* face, int64_t N,
                               float* normals, void* stream);

/* ---- mesh registration: the point-to-plane normal equations of points against the faces a mesh distance query gave them, summed
 * in a fixed order (no counterpart in the reference; csrc/mesh_register.hip).  tests/mesh_register_reference.py restates it in
 * numpy; the kernels match it bit for bit.
 *
 * points [N][3] float32, face [N] int32 and d2 [N] float32 as rtgs_mesh_distance_query wrote them for these points, src_normals
 * [N][3] float32 or NULL, vertices / V / faces / F the query's mesh (the CALLER guarantees 0 <= faces[.] < V), center_host 3 floats
 * on the HOST.  Correspondence i TAKES PART when all of
 *   0 <= face[i] < F;
 *   d2[i] <= max_d2, compared in float32 (equality keeps it, a NaN drops it);
 *   n != (0, 0, 0), n the unit normal of face[i] exactly as rtgs_mesh_distance_normals forms it (one shared device function);
 *   with src_normals: |(s.x n.x + s.y n.y) + s.z n.z| >= min_cos, s = src_normals[i], every step one rounded float32 operation.
 * Its terms are float64, every step one rounded operation on the float32 inputs widened: a = the face's first corner,
 *   q = p - center,  e = p - a,  r = (n.x e.x + n.y e.y) + n.z e.z,
 *   J = (q.y n.z - q.z n.y,  q.z n.x - q.x n.z,  q.x n.y - q.y n.x,  n.x, n.y, n.z),
 *   t[0..20] = J[i] J[j] for i <= j, row-major;  t[21..26] = J[i] r;  t[27] = r r;  t[28] = d2[i];  t[29] = 1.
 * A correspondence that does not take part has t = +0.  out [30] float64 on the device = the sum of t over i in THIS order, which
 * depends on N alone (not on the grid, the number of CUs or any arrival order; there are no float atomics):
 *   chunk  point i belongs to chunk i / C, C = RTGS_MESH_REGISTER_CHUNK = 1024.  Slot s (0..255) of a chunk starts at +0 and adds
 *          the points C chunk + s, + 256, + 512, + 768 (those below N) in that order.
 *   tree   256 slots -> one value: slots 64 w .. 64 w + 63 are wave w; inside a wave x[l] = x[l] + x[l + o] for l < o, with
 *          o = 32, 16, 8, 4, 2, 1 in turn, leaves the wave's value in x[0]; the four waves give (w0 + w1) + (w2 + w3).
 *   total  a second launch of one workgroup: slot s starts at +0 and adds the chunk values s, s + 256, s + 512, ... in that
 *          order, then the same tree.
 * N == 0 writes 30 zeros.  scratch: rtgs_mesh_register_scratch_bytes(N) bytes (the chunk values; 0 for N <= 0), the caller's,
 * 8-byte aligned, reusable by the next call.  Two launches on `stream`, no host read.
 * Return 0, -1 on a bad argument (N < 0 or >= 2^31, V or F <= 0, a null pointer that is needed), -2 on a launch failure. */
#define RTGS_MESH_REGISTER_CHUNK 1024
#define RTGS_MESH_REGISTER_OUT 30
size_t rtgs_mesh_register_scratch_bytes(int64_t N);
int rtgs_mesh_register_accumulate(const float* points, const int32_t* face, const float* d2, const float* src_normals, int64_t N,
                                  const float* vertices, int64_t V, const int32_t* faces, int64_t F, const float* center_host,
                                  float max_d2, float min_cos, void* scratch, double* out, void* stream);

/* ---- mesh texture: a per-face texture atlas of an indexed triangle mesh, baked from colour views (no counterpart in the
 * reference; csrc/mesh_texture.hip).  tests/mesh_texture_reference.py restates every step in numpy; the kernels match it bit for
 * bit.  Float32 throughout, one correctly rounded operation per step, in the order written.  vertices [V][3] float32; faces [F][3]
 * int32, the CALLER guarantees 0 <= faces[i] < V.  u.v = (ux vx + uy vy) + uz vz.
 *
 * rtgs_mesh_texture_levels.  A face gets a square block of s = 2^l texels a side, l in 1..max_level (max_level in
 *   1..RTGS_MESH_TEXTURE_MAX_LEVEL): with L = max(max(|B - A|^2, |C - B|^2), |A - C|^2), d = q - p, |d|^2 = d.d, levels[f] is the
 *   smallest l with t t >= L, t = (float)(s - 1) texel.  Without such an l: levels[f] = max_level, capped[f] = 1 (else 0).  A face
 *   with a non-finite corner coordinate has level 1 and is not capped.  texel > 0 and finite.
 * The CALLER lays the blocks out: faces sorted by level descending, stable in the face index (order [F] int32: the face of every
 *   sorted slot); sorted_offset [F] int64 the exclusive prefix sum of 4^l over that order, T the sum; offset [F] int64 the same per
 *   face.  A block's origin (x0, y0) is the Morton decode of its offset (even bits x0, odd bits y0); the atlas is Wt x Ht, both
 *   <= RTGS_MESH_TEXTURE_MAX_SIDE: k the smallest integer with 4^k >= T, Wt = 2^k, Ht = 2^k when T > 2^(2k-1), else 2^(k-1).
 * rtgs_mesh_texture_face_layout.  origin [F][2] int32 = (x0, y0); uv [F][3][2] float32 = the corners at texel centres,
 *   ((x0 + 0.5) / Wt, (y0 + 0.5) / Ht), (((x0 + s) - 0.5) / Wt, .), (., ((y0 + s) - 0.5) / Ht); record [F][12] float32, 16-byte
 *   aligned, what rtgs_mesh_texture_bake_view reads of a face: A, B - A, C - A (9 floats), then x0, y0 and l as int32 bits.
 * rtgs_mesh_texture_texel_face.  texel_face [Ht][Wt] int32: with c the Morton code of (x, y), -1 when c >= T, else
 *   order[the last slot whose sorted_offset <= c] (a binary search).  F >= 1.
 * A texel's surface point: i = x - x0, j = y - y0; when i + j > s - 1, (i, j) <- (s - 1 - j, s - 1 - i) (the reflection across
 *   the hypotenuse); a = (float)i / (float)(s - 1), b = (float)j / (float)(s - 1); P = (A + a (B - A)) + b (C - A) per component.
 * rtgs_mesh_texture_bake_view.  record as rtgs_mesh_texture_face_layout wrote it, color [3][H][W] float32, depth [H][W] float32 (the depth map of THIS mesh at the view's pose),
 *   w2c12_host as rtgs_visibility_add's, centre_host = the camera centre in the mesh's frame (3 floats on the HOST), acc
 *   [Ht][Wt][4] float32, 16-byte aligned, ZEROED by the caller before the first view.  Per texel with texel_face >= 0:
 *     1  xc, yc, zc and u, v of P: steps 1 and 3 of rtgs_visibility_add; fail unless zc > 0
 *     2  x0 = floorf(u), y0 = floorf(v); fail unless 0 <= x0 <= W - 2 and 0 <= y0 <= H - 2 (the bilinear footprint)
 *     3  d = depth[floorf(v + 0.5f)][floorf(u + 0.5f)]; fail unless d > 0; fail when zc - d > tolerance
 *     4  n = (B - A) x (C - A), r = centre - P, cos2 = ((n.r) (n.r)) / ((n.n) (r.r)); fail unless cos2 >= min_cos2
 *     5  w = cos2 / (zc zc); tx = u - x0, ty = v - y0; per channel top = c00 + tx (c10 - c00), bot = c01 + tx (c11 - c01),
 *        val = top + ty (bot - top); acc.rgb = acc.rgb + w val, acc.w = acc.w + w
 *   Every comparison is false for NaN.  acc[texel] has one owner: no atomics; views add up in the order of the calls.
 * rtgs_mesh_texture_finish.  image [Ht][Wt][3] uint8, flags [Ht][Wt] uint8.  texel_face < 0: colour 0, flag 0.  acc.w > 0: colour
 *   acc.rgb / acc.w, flag 2.  Otherwise flag 1 and the colour (cA + a (cB - cA)) + b (cC - cA) of the face's rows of colors [V][3]
 *   float32, or 0.5 when colors is NULL.  A byte is floorf(c 255 + 0.5f) clamped by fminf(fmaxf(., 0), 255) (NaN gives 0).
 * One launch each, no host read.  Return 0 (also, without a launch, for F == 0 in levels and face_layout), -1 on a bad argument,
 * -2 on a launch failure. */
#define RTGS_MESH_TEXTURE_MAX_LEVEL 6
#define RTGS_MESH_TEXTURE_MAX_SIDE 16384
int rtgs_mesh_texture_levels(const float* vertices, const int32_t* faces, int64_t F, float texel, int32_t max_level, int32_t* levels,
                             int32_t* capped, void* stream);
int rtgs_mesh_texture_face_layout(const float* vertices, const int32_t* faces, const int64_t* offset, const int32_t* levels, int64_t F,
                                  int32_t Wt, int32_t Ht, int32_t* origin, float* uv, float* record, void* stream);
int rtgs_mesh_texture_texel_face(const int64_t* sorted_offset, const int32_t* order, int64_t F, int64_t T, int32_t Wt, int32_t Ht,
                                 int32_t* texel_face, void* stream);
int rtgs_mesh_texture_bake_view(const int32_t* texel_face, int32_t Wt, int32_t Ht, const float* record, const float* color,
                                const float* depth, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                                const float* w2c12_host, const float* centre_host, float tolerance, float min_cos2, float* acc,
                                void* stream);
int rtgs_mesh_texture_finish(const int32_t* texel_face, int32_t Wt, int32_t Ht, const int32_t* faces, const int32_t* levels,
                             const int32_t* origin, const float* colors, const float* acc, uint8_t* image, uint8_t* flags,
                             void* stream);

/* ---- map exposure: every frame's colour in the map's exposure (rtg_slam_amd/map_exposure.py, off by default) ---------------- */
/* A gain alpha and an offset beta per frame take the frame's colour into the exposure of the map, which frame 0 defines.  They are
 * fitted on the pixels where the frame and the map rendered at the frame's pose see the same surface; tests/map_exposure_reference.py
 * is the definition, matched bit for bit.  state: RTGS_MAP_EXPOSURE_STATE doubles on the device, owned by the caller and
 * initialised to (1, 0, 1, 0, 0, ...): alpha, beta, the (alpha, beta) the current frame started from, the code of its fit (0
 * accepted, 1 fewer than min_valid valid pixels, 2 no weight, 3 no variance of intensity, 4 not finite, 5 outside
 * 0.25 <= alpha <= 4, |beta| <= 0.5), the iterations accepted for it, two spare, and at RTGS_MAP_EXPOSURE_SUMS_AT the eight sums of
 * the last iteration that ran: sum w, w I, w R, w I I, w I R, w r r, the valid pixels, those with |r| <= huber.
 * fit.  ONE iteration: colours [3][H][W], depths and T_map [H][W] float32.  A pixel is valid when (float32, false for NaN) frame
 *   depth > 0, render depth > 0, |difference| <= depth_gate, T <= t_gate, lo <= every frame channel <= hi, every render channel
 *   finite.  I, R = (0.299 r + 0.587 g) + 0.114 b of frame and render; Ic = (float)alpha I, Ic = Ic + (float)beta, r = Ic - R,
 *   a = |r|; w = 1 when a <= huber else huber / a, and from iteration 1 on 0 where a > cut huber.  The sums are float64 in a fixed
 *   order (chunks of 1024 pixels, a shuffle / LDS tree, the chunk sums in index order: two runs give the same bits); the solve
 *   det = S0 S3 - S1 S1, alpha = (S0 S4 - S1 S2) / det, beta = (S2 - alpha S1) / S0 and the tests S6 >= min_valid, S0 > 0,
 *   det > var_min S0 S0, finite, in range run at the tail of the second launch.  iteration 0 begins a frame: it records the state
 *   as the frame's start and clears the code.  A rejected iteration restores the start and keeps its code; later iterations of the
 *   frame (iteration > 0) then change nothing.  scratch: device, at least scratch_bytes(H, W), which is 0 for a size that is refused.
 * apply.  out = fminf(fmaxf((float)alpha c + (float)beta, 0), 1), two rounded steps, written as [3][H][W] AND as [H][W][3] in one
 *   launch; the outputs must not be the input.
 * No host read, no atomics.  Return 0, -1 without a launch (null pointer, H or W <= 0, H W >= 2^31, iteration < 0, huber <= 0,
 * cut < 1, depth_gate < 0, lo > hi, var_min < 0, min_valid < 1, a NaN), -2 on a launch failure. */
#define RTGS_MAP_EXPOSURE_STATE 16
#define RTGS_MAP_EXPOSURE_SUMS 8
#define RTGS_MAP_EXPOSURE_SUMS_AT 8
size_t rtgs_map_exposure_scratch_bytes(int32_t H, int32_t W);
int rtgs_map_exposure_fit(const float* frame_color_chw, const float* frame_depth, const float* render_color_chw,
                          const float* render_depth, const float* T_map, int32_t H, int32_t W, int32_t iteration, float huber,
                          float cut, float depth_gate, float t_gate, float lo, float hi, double var_min, int64_t min_valid,
                          double* state, void* scratch, void* stream);
int rtgs_map_exposure_apply(const float* color_chw, int32_t H, int32_t W, const double* state, float* out_chw, float* out_hwc,
                            void* stream);

/* ---- white balance: a gain and an offset per colour channel from one picture to another (csrc/white_balance.hip) ------------- */
/* The map exposure fit above, four regressions at once: k = 0 on the greys (0.299 r + 0.587 g) + 0.114 b exactly as above, k = 1..3
 * on the red, green and blue channels themselves.  It serves the mapper (source = frame, target = the map's render;
 * map_exposure_channels: rgb) and the exposure-aware evaluation (source = the map's render, target = the frame).
 * tests/white_balance_reference.py is the definition, matched bit for bit.
 * state: RTGS_WHITE_BALANCE_STATE doubles on the device, owned by the caller.  Regression k owns the RTGS_WHITE_BALANCE_REG doubles
 * from RTGS_WHITE_BALANCE_REG k: alpha, beta, the (alpha, beta) the current frame started from, its code (the codes above; 3 reads
 * "no variance of the source"), the iterations accepted for it, two spare; the caller initialises each to (1, 0, 1, 0, 0, ...).  At
 * RTGS_WHITE_BALANCE_FRAME_AT the frame's code and seven spare; at RTGS_WHITE_BALANCE_SUMS_AT the RTGS_WHITE_BALANCE_SUMS sums of the
 * last iteration that ran: at 7 k + j of regression k sum w, w s, w t, w s s, w s t, w r r and the pixels with |r| <= huber, at 28 the
 * valid pixels, then three that stay +0.
 * fit.  ONE iteration: colours [3][H][W], depths and T_map [H][W] float32.  A pixel is valid when (float32, false for NaN) source
 *   depth > 0, target depth > 0, |difference| <= depth_gate, T <= t_gate, src_lo <= every source channel <= src_hi, dst_lo <= every
 *   target channel <= dst_hi, all six finite (the bounds may be infinite).  Per regression, with s and t its source and target
 *   value: r = ((float)alpha_k s + (float)beta_k) - t in two rounded steps, a = |r|, w = 1 when a <= huber else huber / a, and from
 *   iteration 1 on 0 where a > cut huber.  The sums are float64 in the fixed order of the map exposure fit; the solve and its tests
 *   run per regression as above, S28 >= min_valid first.  iteration 0 begins a frame: every regression records its state as the
 *   frame's start, all codes are cleared.  The frame rule: a refused grey regression (too few valid pixels refuses all four) ends
 *   the frame's fit - all four return to the frame's start, the frame's code is the grey's, a channel without a code takes its own
 *   of this iteration, and later iterations of the frame (iteration > 0) change nothing.  Otherwise a channel whose own
 *   regression is refused takes the grey's (alpha, beta) of this iteration, keeps its code and follows the grey, unsolved, for the
 *   rest of the frame; the frame's code stays 0.  scratch: device, at least scratch_bytes(H, W), 0 for a size that is refused.
 * apply.  out_c = fminf(fmaxf((float)alpha_c c + (float)beta_c, 0), 1) for c = 1..3 (the grey regression is not used), written as
 *   [3][H][W] AND as [H][W][3] in one launch; the outputs must not be the input.
 * No host read, no atomics.  Return 0, -1 without a launch (null pointer, H or W <= 0, H W >= 2^31, iteration < 0, huber <= 0,
 * cut < 1, depth_gate < 0, src_lo > src_hi, dst_lo > dst_hi, var_min < 0, min_valid < 1, a NaN), -2 on a launch failure. */
#define RTGS_WHITE_BALANCE_REGRESSIONS 4
#define RTGS_WHITE_BALANCE_REG 8
#define RTGS_WHITE_BALANCE_FRAME_AT 32
#define RTGS_WHITE_BALANCE_SUMS_AT 40
#define RTGS_WHITE_BALANCE_SUMS 32
#define RTGS_WHITE_BALANCE_VALID 28
#define RTGS_WHITE_BALANCE_STATE 72
size_t rtgs_white_balance_scratch_bytes(int32_t H, int32_t W);
int rtgs_white_balance_fit(const float* src_color_chw, const float* src_depth, const float* dst_color_chw, const float* dst_depth,
                           const float* T_map, int32_t H, int32_t W, int32_t iteration, float huber, float cut, float depth_gate,
                           float t_gate, float src_lo, float src_hi, float dst_lo, float dst_hi, double var_min, int64_t min_valid,
                           double* state, void* scratch, void* stream);
int rtgs_white_balance_apply(const float* color_chw, int32_t H, int32_t W, const double* state, float* out_chw, float* out_hwc,
                             void* stream);

/* ---- loop closure: the map moves with its frames (no counterpart in the reference, whose ORB back end corrects poses only;
 * csrc/map_deform.hip).  tests/map_deform_reference.py restates it in numpy float32; the kernel matches it bit for bit.
 *
 * rtgs_map_deform.  xyz [N][3] and raw8 [N][8] (raw opacity | 3 log scales | rotation quaternion w x y z) float32, updated IN
 *   PLACE; tick [N] = the frame that added the row, int32 (tick_kind 0) or int64 (tick_kind 1); table [n_frames][16] float32,
 *   16-B aligned: per frame the correction D(f) as the 3 rows of its 3 x 4 matrix (r00 r01 r02 t0 | r10 .. | r20 ..), then its
 *   unit quaternion (w, x, y, z) - built on the host in float64 and rounded.  Per row, one lane, float32:
 *     1  f = tick clamped to [0, n_frames - 1]; the 16 values of table[f]
 *     2  if all 16 compare equal to the identity's (1 0 0 0 | 0 1 0 0 | 0 0 1 0 | 1 0 0 0) the row is NOT written: it stays
 *        bit-identical, -0.0 included
 *     3  x' = fmaf(r00, x, fmaf(r01, y, fmaf(r02, z, t0))), y' and z' likewise from rows 1 and 2
 *     4  q' = q_D (x) q_raw, the Hamilton product, a = q_D, b = q_raw:
 *          w' = fmaf(-az, bz, fmaf(-ay, by, fmaf(-ax, bx, aw bw)))     x' = fmaf(-az, by, fmaf(ay, bz, fmaf(ax, bw, aw bx)))
 *          y' = fmaf(az, bx, fmaf(ay, bw, fmaf(-ax, bz, aw by)))       z' = fmaf(az, bw, fmaf(-ay, bx, fmaf(ax, by, aw bz)))
 *        not normalised: the raw quaternion keeps its norm up to the rounding of a unit q_D
 *   Opacity, scales and the SH block are not touched (the higher SH bands are NOT rotated unless loop_closure_rotate_sh: then
 *   rtgs_map_deform_sh below turns them behind this call).  No atomics, no host read, two runs
 *   are bit-equal.  Returns 0 (also, without a launch, for N == 0), -1 on a null or misaligned pointer, N < 0 or above
 *   RTGS_MAP_DEFORM_MAX_ROWS, n_frames < 1 or an unknown tick_kind, -2 on a launch failure. */
#define RTGS_MAP_DEFORM_MAX_ROWS 2147483647LL
int rtgs_map_deform(float* xyz, float* raw8, const void* tick, int32_t tick_kind, int64_t N, const float* table,
                    int32_t n_frames, void* stream);

/* rtgs_map_deform_sh (csrc/map_deform_sh.hip).  The higher SH bands of the same rows turn with the correction's rotation.
 *   shs [N][16][3] float32 (coefficient-major, channel-minor), 16-B aligned, updated IN PLACE; tick, tick_kind and the clamp of f
 *   as above; sh_table [n_frames][84] float32, 16-B aligned (336 B a row): per frame the matrices M1 [3][3], M2 [5][5], M3 [7][7]
 *   with Y_l(R d) = M_l Y_l(d) for the basis functions of the rasterizer (rtg_slam_amd/sh_rotation.py, built on the host in
 *   float64 and rounded), row-major, 9 + 25 + 49 values, then one flag.  Per row, float32:
 *     1  f = tick clamped to [0, n_frames - 1]
 *     2  if the flag sh_table[f][83] compares equal to 0 the row is NOT written: it stays bit-identical, -0.0 included
 *     3  coefficient 0 is not touched; for each band (coefficients 1..3, 4..8, 9..15: n = 3, 5, 7), each output i and each channel,
 *        with x the band's n coefficients of that channel:
 *          acc = M[i][n-1] * x[n-1];   for j = n-2 .. 0:  acc = fmaf(M[i][j], x[j], acc);   coefficient (first + i) = acc
 *   tests/map_deform_sh_reference.py restates it in numpy float32; the kernel matches it bit for bit.  No atomics, no host read,
 *   two runs are bit-equal.  Returns 0 (also, without a launch, for N == 0), -1 on a null or misaligned pointer, N < 0 or above
 *   RTGS_MAP_DEFORM_MAX_ROWS, n_frames < 1 or an unknown tick_kind, -2 on a launch failure. */
int rtgs_map_deform_sh(float* shs, const void* tick, int32_t tick_kind, int64_t N, const float* sh_table, int32_t n_frames,
                       void* stream);

/* ---- loop closure: place recognition by appearance (no counterpart in the reference, whose ORB back end recognises places by a
 * trained vocabulary; csrc/place.hip).  tests/place_reference.py is the definition, in numpy; both kernels match it bit for bit.
 * Every float64 sum is taken in THE WAVE ORDER over a flat list v[0 .. n - 1]: lane l of 64 adds v[l], v[l + 64], ... in that
 * order onto +0.0, then six butterfly steps o = 32, 16, .. 1 replace each lane's value by its own plus that of lane l ^ o
 * (the tree t[:o] = t[:o] + t[o:2o]); a missing or gated-out element counts as +0.0.
 *
 * rtgs_place_describe.  One keyframe: color_chw [3][H][W] and depth [H][W] float32 -> one row of tw th cells, row by row, of each
 *   of the caller's descriptor arrays.  Cell (i, j) covers rows floor(i H / th) .. floor((i + 1) H / th) - 1 and columns
 *   floor(j W / tw) .. floor((j + 1) W / tw) - 1, n pixels; its flat list runs over them row by row.
 *     intensity = (float)(sum(grey) / n), grey = (0.299f r + 0.587f g) + 0.114f b in float32, not contracted
 *     depth     = (float)(sum(z over z > 0) / count(z > 0)), 0 without such a pixel
 *     valid     = (float)((double)count / (double)n); a cell is depth-valid when valid >= 0.5f
 *   One wave per cell.  Returns 0, -1 without a launch (null pointer, H or W < 1, H W >= 2^31, tw or th < 1, tw > W, th > H,
 *   tw th > RTGS_PLACE_MAX_CELLS), -2 on a launch failure.
 *
 * rtgs_place_scores.  intensity, depth, valid [M][th tw] float32; score, depth_rel float32 and shift int32 [M][M], indexed
 *   [b][a]: row b holds keyframe b against every older keyframe a.  Rows b_begin <= b < b_end are written in full, no other
 *   row is touched: for a <= b - min_gap the pair's figures, for every other a the sentinels -2, 0, +inf.
 *   A pair at the shift s, |s| <= S: column x of a against column x + s of b, x0 = max(0, -s) <= x < x0 + ow, ow = tw - |s|,
 *   all rows; the flat list runs over the overlap row by row, n = th ow cells.  A, B the grey cells as float64:
 *     SA, SB, SAA, SBB, SAB = sums of A, B, A A, B B, A B       ma = SA / n, mb = SB / n
 *     va = SAA / n - ma ma, vb = SBB / n - mb mb, cov = SAB / n - ma mb       (float64, not contracted)
 *     zncc = -1 if va <= 1e-12 or vb <= 1e-12, else cov / sqrt(va vb)
 *   The shifts are visited as 0, -1, +1, -2, +2, ..; a later one wins only if strictly greater.  score = (float)best.  At that
 *   shift, over the same list and the cells depth-valid in both: depth_rel = (float)(sum|da - db| / (0.5 sum(da + db))), +inf
 *   when 4 count < n.  One wave per pair; both grey thumbnails are read once, into LDS, for all shifts.
 *   Returns 0 (also, without a launch, for b_begin == b_end), -1 without a launch (null pointer, M < 1 or above
 *   RTGS_PLACE_MAX_KEYFRAMES, tw or th < 1, tw th > RTGS_PLACE_MAX_CELLS, S < 0, 2 S >= tw, min_gap < 1, b_begin < 0,
 *   b_begin > b_end, b_end > M), -2 on a launch failure.
 * No atomics, no host read, two runs are bit-equal.  No alignment beyond float's is required. */
#define RTGS_PLACE_MAX_CELLS 2048
#define RTGS_PLACE_MAX_KEYFRAMES 16384
int rtgs_place_describe(const float* color_chw, const float* depth, int32_t H, int32_t W, int32_t tw, int32_t th,
                        float* intensity_out, float* depth_out, float* valid_out, void* stream);
int rtgs_place_scores(const float* intensity, const float* depth, const float* valid, int32_t M, int32_t tw, int32_t th, int32_t S,
                      int32_t min_gap, int32_t b_begin, int32_t b_end, float* score, int32_t* shift, float* depth_rel, void* stream);

/* ---- loop closure: a relative pose for a wide-baseline revisit from matched keypoints (the reference gets it from its ORB back
 * end, use_orb_backend; csrc/keypoints.hip).  tests/keypoint_reference.py is the definition, in numpy; after the grey value
 * everything is integer arithmetic and the three kernels match it bit for bit.
 *
 * rtgs_keypoint_detect.  One keyframe: color_chw [3][H][W] and depth [H][W] float32 ->
 *     g8    [H][W] uint8:  clamp(floor(grey 255 + 0.5), 0, 255), grey = (0.299f r + 0.587f g) + 0.114f b in float32, not contracted;
 *     box5  [H][W] int32:  the 5 x 5 sum of g8 around the pixel, pixels outside the image counting as 0;
 *     slots [ceil(H / cell) ceil(W / cell)][4] int32, cells row by row: x, y, score of the cell's keypoint and -1; 0, 0, 0, -1
 *           for a cell without one.
 *   score is the FAST-9 score on the circle of radius 3 (the largest threshold at which the pixel is still a corner); a pixel is
 *   eligible when score > threshold, RTGS_KEYPOINT_MARGIN <= x < W - RTGS_KEYPOINT_MARGIN, the same for y, and its depth is
 *   finite and > 0, and counts as 0 otherwise; it survives the 3 x 3 suppression when its score is strictly greater than those
 *   of the four neighbours earlier in raster order and at least those of the four later; a cell keeps the survivor of the
 *   highest score, on a tie the one with the lowest row-major pixel index.  One block per cell.
 *   Returns 0, -1 without a launch (null pointer, H or W < 1, H W >= 2^31, cell outside RTGS_KEYPOINT_MIN_CELL ..
 *   RTGS_KEYPOINT_MAX_CELL, threshold outside 0 .. 255, more than 65535 rows of cells), -2 on a launch failure.
 *
 * rtgs_keypoint_describe.  g8, box5 and slots of rtgs_keypoint_detect (n_slots of them) -> slots[.][3] = the orientation bin and
 *   desc [n_slots][8] uint32; -1 and zeros for an empty slot.  m10 = sum dx g8, m01 = sum dy g8 over dx^2 + dy^2 <= 169;
 *   bin = argmax_k (dirs[k][0] m10 + dirs[k][1] m01) over k = 0 .. 31 in int64, ties to the lowest k; bin 0 when oriented == 0.
 *   Bit i of the descriptor (word i / 32, position i % 32) is box5(keypoint + P1) < box5(keypoint + P2) with
 *   tables[bin][i] = the four int8 x1, y1, x2, y2 packed into one word, lowest byte first.  dirs [32][2] int32 and tables
 *   [32][256] uint32 are device buffers the host builds once (rtg_slam_amd/keypoints.py), so that the kernel and the definition
 *   read the same numbers.  One wave per slot.
 *   Returns 0 (also, without a launch, for n_slots == 0), -1 (null pointer, H or W < 1, H W >= 2^31, n_slots < 0), -2.
 *
 * rtgs_keypoint_match.  desc [n_desc][8] uint32, 16-byte aligned, holds the descriptors of all keyframes; pairs [n_pairs][5] int32
 *   (device) = first query row, query count, first reference row, reference count, first row of `out`; out [n_out][3] int32.
 *   For query q of a pair, out[first + q] = the reference index (within its set) of the least Hamming distance, ties to the
 *   lowest index; that distance; the least distance over all other indices of the set, 257 when there is none.  An empty
 *   reference set gives -1, 257, 257.  max_queries is the largest query count (it sizes the grid); a pair whose rows do not lie
 *   inside the buffers is skipped.  One launch for the whole batch, one wave per query.
 *   Returns 0 (also, without a launch, for n_pairs == 0 or max_queries == 0), -1 (null or misaligned pointer, a negative count,
 *   n_pairs > 65535, n_desc or n_out >= 2^31), -2.
 * No atomics, no host read, two runs are bit-equal. */
#define RTGS_KEYPOINT_MARGIN 16
#define RTGS_KEYPOINT_MIN_CELL 8
#define RTGS_KEYPOINT_MAX_CELL 32
int rtgs_keypoint_detect(const float* color_chw, const float* depth, int32_t H, int32_t W, int32_t cell, int32_t threshold,
                         uint8_t* g8, int32_t* box5, int32_t* slots, void* stream);
int rtgs_keypoint_describe(const uint8_t* g8, const int32_t* box5, int32_t H, int32_t W, int32_t n_slots, int32_t oriented,
                           const int32_t* dirs, const uint32_t* tables, int32_t* slots, uint32_t* desc, void* stream);
int rtgs_keypoint_match(const uint32_t* desc, int64_t n_desc, const int32_t* pairs, int32_t n_pairs, int32_t max_queries,
                        int32_t* out, int64_t n_out, void* stream);

/* ---- the keypoints over an image pyramid, so that a revisit from another distance matches, and the votes by which revisits are
 * found (csrc/keypoint_pyramid.hip).  tests/keypoint_pyramid_reference.py is the definition, in numpy; after the grey value
 * everything is integer arithmetic and the four kernels match it bit for bit.
 *
 * THE LADDER.  Level l has the scale num / den = 1, 3/2, 2, 3, 4.  Level 1 is level 0 reduced 3:2, level 2 is level 0 reduced 2:1,
 *   level 3 is level 1 reduced 2:1, level 4 is level 2 reduced 2:1.
 *     2:1  size floor(W / 2) x floor(H / 2), value (a + b + c + d + 2) >> 2 of the 2 x 2 block; a trailing odd row or column is dropped
 *     3:2  size 2 floor(W / 3) x 2 floor(H / 3); along each axis output 2k takes the inputs 3k, 3k + 1 with the weights 2, 1 and
 *          output 2k + 1 the inputs 3k + 1, 3k + 2 with 1, 2; value (sum of the 2-D weight products times g8 + 4) / 9
 *   Level 0's g8 is rtgs_keypoint_detect's.  A level's depth at (x, y) is level 0's at (floor((2x + 1) num / (2 den)),
 *   floor((2y + 1) num / (2 den))): never an average.
 *   levels [n_levels][5] int32 is a HOST array, 1 <= n_levels <= RTGS_KEYPOINT_MAX_LEVELS: first pixel of the level in the
 *   buffers, H, W, num, den.  The caller chooses how many levels and where they lie; H, W, num and den must be the ladder's, every
 *   level must lie inside the n_pixels of the buffers and no two may overlap.
 *
 * rtgs_keypoint_pyramid.  color_chw [3][H][W] and depth [H][W] float32 (H, W = level 0's) -> g8 [n_pixels] uint8 and depth_levels
 *   [n_pixels] float32, the planes of all levels.  One block per 48 x 48 tile of level 0 makes that tile of every level.
 * rtgs_keypoint_detect_levels.  g8, depth_levels -> box5 [n_pixels] int32 (per level, pixels outside the level counting as 0) and
 *   slots [cells][4] int32: the slots of rtgs_keypoint_detect for every level in turn, level after level, x and y in the
 *   level's pixels; cells = sum over the levels of ceil(H_l / cell) ceil(W_l / cell).  The rule per level is rtgs_keypoint_detect's,
 *   the margin counted in the level's pixels.
 * rtgs_keypoint_describe_levels.  rtgs_keypoint_describe over the same slots -> slots[.][3] and desc [cells][8] uint32.
 *   All three return 0, -1 without a launch (null pointer, a table that is not the ladder's or leaves the buffers, n_pixels < 1 or
 *   >= 2^31, cell or threshold outside rtgs_keypoint_detect's ranges), -2 on a launch failure.  With n_levels = 1 the three
 *   together leave what rtgs_keypoint_detect and rtgs_keypoint_describe leave.
 *
 * rtgs_keypoint_votes.  matches [n_matches][3] int32 holds the tables rtgs_keypoint_match wrote; pairs [n_pairs][4] int32 (device),
 *   for the pair (a, b): first row and count nb of the table of b's keypoints against a's, first row and count na of the table
 *   of a's against b's.  votes[pair] = the number of rows i of b's table that survive rtgs_rigid_ransac's filter: 0 <= j < na,
 *   a's row j names i, d <= max_hamming and (double)d <= ratio (double)second; not capped.  A pair whose rows do not lie inside
 *   the buffer is skipped: votes keeps what it held.  One wave per pair, ballots and population counts.
 *   Returns 0 (also, without a launch, for n_pairs == 0), -1 (null pointer, a negative count, n_matches >= 2^31, ratio negative or
 *   NaN), -2.
 * No atomics, no host read, two runs are bit-equal. */
#define RTGS_KEYPOINT_MAX_LEVELS 5
int rtgs_keypoint_pyramid(const float* color_chw, const float* depth, const int32_t* levels, int32_t n_levels, int64_t n_pixels,
                          uint8_t* g8, float* depth_levels, void* stream);
int rtgs_keypoint_detect_levels(const uint8_t* g8, const float* depth_levels, const int32_t* levels, int32_t n_levels, int64_t n_pixels,
                                int32_t cell, int32_t threshold, int32_t* box5, int32_t* slots, void* stream);
int rtgs_keypoint_describe_levels(const uint8_t* g8, const int32_t* box5, const int32_t* levels, int32_t n_levels, int64_t n_pixels,
                                  int32_t cell, int32_t oriented, const int32_t* dirs, const uint32_t* tables, int32_t* slots,
                                  uint32_t* desc, void* stream);
int rtgs_keypoint_votes(const int32_t* matches, int64_t n_matches, const int32_t* pairs, int32_t n_pairs, int32_t max_hamming,
                        double ratio, int32_t* votes, void* stream);

/* ---- the match filter and the 3-D - 3-D rigid RANSAC of a batch of keyframe pairs on the device (csrc/rigid_ransac.hip; on the
 * host it is keypoints.filter_matches and keypoints.ransac_rigid, 512 hypotheses a pair through LAPACK).
 * tests/rigid_ransac_reference.py is the definition, in numpy float64: + - * / and sqrt in a stated order, every sum over matches
 * in THE WAVE ORDER (above), a gated-out match counting as +0.0; the kernel matches it bit for bit.  It is a definition of its
 * own: it fits by Horn's closed form where ransac_rigid uses an SVD, so the two agree to rounding, not in bits.
 *
 * rtgs_rigid_ransac.  matches [n_matches][3] int32 holds the tables rtgs_keypoint_match wrote (index, distance, second); xyz
 *   [n_xyz][3] float64 the keypoints' back-projected points; pairs [n_pairs][6] int32 (device), for the pair (a, b): first row
 *   and count nb of the table of b's keypoints against a's, first row and count na of the table of a's against b's, first row
 *   of a's points and first row of b's points in xyz (na and nb of them).  A pair whose rows do not lie inside the buffers is
 *   skipped: its record keeps what it held.
 *     filter      row i of b's table survives when 0 <= j < na, a's row j names i, d <= max_hamming and (double)d <= ratio
 *                 (double)second; the survivors in order of i, at most RTGS_RANSAC_MAX_MATCHES, are the n matches (a ballot and
 *                 a prefix count, no atomics)
 *     hypothesis  h = 0 .. iters - 1 draws mix32(seed + 3 h + j) mod n, j = 0, 1, 2 (uint32); skipped on a repeated index or
 *                 when, in either frame, not |e1|^2 > 1e-18, not |e2|^2 > 1e-18 or not |e1 x e2|^2 >= 0.01 (|e1|^2 |e2|^2)
 *     fit         of the triplet, and of the inliers in a refit: centroids, the 3 x 3 cross-covariance, Horn's symmetric 4 x 4
 *                 matrix, its dominant eigenvector by 8 cyclic Jacobi sweeps (t = sign(theta) / (|theta| + sqrt(theta^2 + 1)),
 *                 c = 1 / sqrt(t^2 + 1), s = t c, a zero off-diagonal skipped), the normalised quaternion to R, t = c_a - R c_b
 *     count       a match is an inlier when (dx^2 + dy^2) + dz^2 <= inlier_dist^2, d = ((R b) + t) - a; the highest count wins,
 *                 the earliest h on a tie
 *     refit       up to three rounds on the inliers; a round that loses inliers is dropped and ends them, an unchanged set too
 *   out [n_pairs][RTGS_RANSAC_HEAD + 3 max_matches] int32, 8-byte aligned, one record per pair: words 0 .. 33 hold 17 float64 -
 *   T row by row (p_a = T p_b) and the rms of the inliers' residuals; word 34 n, 35 the inlier count, 36 the winning h (-1: no
 *   valid hypothesis, or n < 3 - then T and rms are 0), 37 the survivors before the cap, 38 and 39 zero; then max_matches rows
 *   (i, j, inlier flag), -1, -1, 0 beyond n.  max_matches must be even, at most RTGS_RANSAC_MAX_MATCHES, and at least the
 *   smaller of that and the largest nb, or matches are dropped earlier than the definition drops them.
 *   One block of 256 threads per pair: the n matches' points are staged once in LDS (48 KiB), one lane per hypothesis, the block's
 *   best by shuffles, the refits by wave 0.
 *   Returns 0 (also, without a launch, for n_pairs == 0), -1 without a launch (null or misaligned pointer, a negative count,
 *   n_pairs > 65535, n_matches or n_xyz >= 2^31, iters < 1 or above RTGS_RANSAC_MAX_ITERS, max_matches negative, odd or above
 *   RTGS_RANSAC_MAX_MATCHES, inlier_dist or ratio negative or NaN), -2 on a launch failure.
 * No atomics, no host read, two runs are bit-equal. */
#define RTGS_RANSAC_MAX_MATCHES 1024
#define RTGS_RANSAC_MAX_ITERS 65535
#define RTGS_RANSAC_HEAD 40
int rtgs_rigid_ransac(const int32_t* matches, int64_t n_matches, const double* xyz, int64_t n_xyz, const int32_t* pairs,
                      int32_t n_pairs, int32_t max_hamming, double ratio, int32_t iters, double inlier_dist, uint32_t seed,
                      int32_t max_matches, int32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RTGS_SLAM_H */
