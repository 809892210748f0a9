/* rtgs_debug.h - measurement aids and A-B / test knobs of librtgs_hip.so.
 *
 * NOT part of the drop-in boundary (include/rtgs_raster.h, rtgs_icp.h, rtgs_slam.h): nothing the reference's call sites
 * need lives here.  These entry points exist so that tests can force the paths a workload would pick by itself (fallback
 * sort, near slice on / off, the three backward walks, two-pass binning) and so that bench.py / tools/ can read per-stage
 * timings and work counters.  Every knob is per context (rtgs_ctx); the plain names act on the process-wide default
 * context.  Moved out of rtgs_raster.h in round 5 (VERDICT r4 "weak 11"). */
#ifndef RTGS_DEBUG_H
#define RTGS_DEBUG_H
#include "rtgs_raster.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Device-side counters of work actually done by blend_fwd: per tile, [2 t] = list entries the tile's walk consumed
 * before every pixel had terminated, [2 t + 1] = (entry, pixel) pairs evaluated.  `counters` = device uint64[2 x tiles]
 * (written, not accumulated, by each forward), or NULL to disable.  Per context, sticky until reset with NULL
 * (measurement aid). */
void rtgs_raster_set_counters(void* counters);
void rtgs_raster_set_counters_ctx(rtgs_ctx* ctx, void* counters);

/* Optional per-stage HIP-event timing of the calls made through the context (off by default;
 * measurement aid - the backward of a forward must use the same context for its stages to show up).
 * rtgs_raster_last_timings fills ms12_host[0..11] with the last forward/backward's stage
 * durations in milliseconds (-1 = stage did not run):
 *   [0] preprocess_fwd (+ mask SAT)  [1] bin_count + tilescan (fallback: scan)  [2] bin_scatter
 *   (fallback: emit_keys)  [3] bin_tilesort (fallback: radix sort)  [4] tile_ranges (fallback only)
 *   [5] blend_fwd  [6] blend_bwd (the launches that have lists to walk)  [7] preprocess_bwd
 *   [8] near-slice binning (histogram, count, scan, scatter, sort)  [9] near-slice blend_fwd
 *   [10] grad_reduce (sum of the gradient slots per Gaussian)  [11] unused
 * With the near-slice pass on, [1]..[5] describe the second pass (tiles the slice left unfinished). */
void rtgs_raster_set_profiling(int enable);
void rtgs_raster_set_profiling_ctx(rtgs_ctx* ctx, int enable);

/* Near-slice (occlusion) pass of the forward.  The nearest Gaussians - as many depth bins as fit a budget of
 * `budget_per_tile` x tiles instances - are binned, sorted and blended first; a tile whose every pixel reaches
 * T < T_threshold inside that slice is final (the slice list is a prefix of the tile's full depth-ordered list, so
 * the walk would have stopped there anyway); only the other tiles are binned against the whole map.  Outputs are
 * bit-identical to the single-pass forward; the backward walks each tile's list of the pass that finished it.
 * mode 0 = off, 1 = always, 2 = automatic (default): considered for maps of >= 100 000 Gaussians on >= 256 tiles, and
 * there the kernels decide from the depth histograms of THIS call (no history): the slice runs only if its Gaussians
 * carry enough optical depth to saturate the image (sum of radius^2 >= 24 per pixel) and the map holds at least twice
 * the slice's instances; otherwise the slice is empty and every tile goes to the second pass.  budget_per_tile <= 0
 * keeps the current budget (default 384).  Environment overrides at load time: RTGS_NEAR_SLICE, RTGS_NEAR_SLICE_BUDGET.
 * rtgs_raster_last_slice_stats: [0] slice used by the last forward, [1] instances binned for the slice,
 * [2] tiles it finished, [3] tiles left to the second pass. */
void rtgs_raster_set_near_slice(int mode, int budget_per_tile);
void rtgs_raster_set_near_slice_ctx(rtgs_ctx* ctx, int mode, int budget_per_tile);

/* Testing aid: force the fallback binning path (global 64-bit radix sort, rocPRIM) that is
 * otherwise taken only when the tile grid or one tile list exceeds the LDS-resident path. */
void rtgs_raster_force_sort_path(int enable);
void rtgs_raster_force_sort_path_ctx(rtgs_ctx* ctx, int enable);
int rtgs_raster_last_timings(float* ms12_host);
int rtgs_raster_last_timings_ctx(rtgs_ctx* ctx, float* ms12_host);

/* The backward's tile walk.  Three kernels exist (raster_bwd.hip, raster_bwd_entry.hip):
 *  - entry-per-lane walk (default): a lane holds one (pixel, ENTRY) pair - 16 entries x 4 pixels per wave step - T and the
 *    colour behind are in-row DPP scans, and the sums over the pixels are kept per lane;
 *  - strip walk: pixel per lane, one entry per wave pass, tile-uniform (large footprints);
 *  - row-granular walk: pixel per lane, every 4x4 block walks its own sub-list (small footprints).
 * mode 0 (default) and 3 = entry-per-lane walk on every tile; 1 = strip walk; 2 = row-granular walk; 4 = per-tile choice between
 * strip and row-granular from the share of the tile's list its 4x4 blocks need (ROWS_MAX_SHARE, raster_common.h) - the
 * round-3 behaviour, kept for A-B runs.  RTGS_BWD_WALK at load time.  Gradients of the walks agree to float rounding.
 * rtgs_raster_image_offsets: byte offsets inside the image buffer - [0] tile ranges (uint2 per tile), [1] n_contrib
 * (u32 per pixel), [2] BwdInfo, [3] tile walk (u32 per tile: bits 0..1 = 0 strip / 1 row-granular / 2 entry-per-lane, bits 8.. the
 * measured share in 1/1000), [4] total size, [5] list position of every pixel's depth owner (u32 per pixel). */
void rtgs_raster_set_bwd_walk_ctx(rtgs_ctx* ctx, int mode);
/* One-pass binning (round 4; default on, RTGS_BIN_ONEPASS=0 at load time turns it off): where the geometry buffer gives
 * every tile a segment (maps of >= 100 000 Gaussians on >= 256 tiles), instances are placed by ONE enumeration sweep
 * (bin_place_kernel) instead of count + scan + scatter.  Outputs are bit-identical either way (the tile sort's order is
 * total); the switch exists for A-B runs and tests. */
void rtgs_raster_set_onepass_ctx(rtgs_ctx* ctx, int on);
/* Near-slice forward: the blend's workgroup sorts its tile's list itself (default on, RTGS_FWD_SORT=0 at load time turns it
 * off: the sort launches in front of the blend, as before).  Lists of up to 1 024 entries are sorted in the blend's LDS
 * (bitonic up to 256, LSD radix above); lists of 1 025 .. 3 072 entries keep one sort launch ahead of the blend; longer ones
 * leave their tile to pass 2 either way.  The order is total, so the lists - and every output - are the same either way; the
 * switch exists for A-B runs and tests, and forgets the speculative plan.
 * rtgs_raster_fused_sort_stats_ctx: out18 = six classes x (tiles, shortest list, longest list) of the last near-slice blend that
 * ran fused WITH work counters set (rtgs_raster_set_counters_ctx; the product kernel keeps no such words) - empty, single,
 * bitonic, fused radix, separate launch, left to pass 2.  Waits for the device. */
void rtgs_raster_set_fused_sort_ctx(rtgs_ctx* ctx, int on);
int rtgs_raster_fused_sort_stats_ctx(rtgs_ctx* ctx, int64_t* out18);
/* Near-slice forward of the speculative map step (kind 1: the slice finished every tile last time): the blend's workgroups
 * gather their own lists.  The list-form shade appends one 4-byte word per tile ROW of a live Gaussian's rect to that row's
 * band (x0 | x1 << 8 | list position << 16, in the bucket nobody else uses on this path); the tile's workgroup scans its row's
 * band, keeps the entries whose column range holds it, runs bin_place's own test on them, and sorts what is left - bin_place
 * and the sort launch in front of the blend are not launched.  Same lists, same counts, same outputs.
 * mode 0 = off, 1 = automatic (default): taken when the structure allows it (per-tile segments, fused sort, at most 255 tile
 * columns and 256 tile rows, the bands fit the bucket), the last verified work list is within the slice's Gaussian budget and the
 * decayed longest slice list is at most 7/8 of the 1 024 entries the blend sorts; 2 = forced (tests): whatever those two are.
 * A tile that finds more than 1 024 hits leaves itself to pass 2, the guess "every tile finished" fails, and the step is redone
 * classically; that call reports the list, and in both modes the path then stays off while the reported (decaying) maximum is
 * above 1 024.  RTGS_TILE_GATHER at load time; the setter forgets the speculative plan.
 * rtgs_raster_tile_gather_stats_ctx: out6 = forwards that gathered | speculative kind-1 forwards on segments with the fused sort
 * that did not: work list too long | longest list too long | layout; band entries scanned per round | candidates a round keeps. */
void rtgs_raster_set_tile_gather_ctx(rtgs_ctx* ctx, int mode);
int rtgs_raster_tile_gather_stats_ctx(rtgs_ctx* ctx, int64_t* out6);
/* Timing decompositions of the entry-per-lane backward walk (tools only): bits 0..2 switch parts of the kernel OFF (1 walk,
 * 2 depth partials, 4 stores) - results are then wrong by construction, so the bits are never read from the environment and a
 * tool that sets them clears them again.  PROCESS-WIDE. */
void rtgs_raster_set_bwd_debug(int bits);
/* Per-wave time stamps of the entry-per-lane backward walk (tools/bwd_stamps.py): `dev` = device uint64[tiles x 4 waves x 14] or NULL
 * (default: the product kernel carries no stamping code).  Per wave: wall clock (100 MHz) at entry and exit, shader cycles
 * in the group loop and in the kernel, groups walked, quad steps entered, cycles of the six other phases.  PROCESS-WIDE; the
 * caller keeps the buffer alive until it has passed NULL again. */
void rtgs_raster_set_bwd_stamps(void* dev);
/* The same for blend_fwd (tools/fwd_stamps.py): `dev` = device uint64[tiles x 4 waves x 8]: wall clock at entry / exit, cycles until
 * the tile range is there | until the first batch is staged | inside the walk loops | in the kernel, walk steps, batches. */
void rtgs_raster_set_fwd_stamps(void* dev);
/* The same for the tracker's residual launches (tools/icp_stamps.py): `dev` = device uint64[RTGS_ICP_STAMP_LAUNCHES x
 * RTGS_ICP_STAMP_WGS workgroups x 4 waves x 8] or NULL.  Residual launch k after the call (rtgs_icp_track, rtgs_icp_step) takes
 * slot k % RTGS_ICP_STAMP_LAUNCHES and runs the stamped twin of the kernel.  Per wave: wall clock (100 MHz) at entry and exit,
 * shader cycles of the source loads | gathers | projection, gates and sums | the partial row's store | the head's reads of
 * the previous launch's rows + float64 sum | its solve, both of the wave's own workgroup (head-solve chain, the default;
 * zero in a track's first launch).  With RTGS_ICP_FLAG_LAST_ARRIVER: ... | partial publish + ticket | last arriver's partial
 * reads + float64 sum | its solve.  PROCESS-WIDE; each call restarts at slot 0. */
#define RTGS_ICP_STAMP_LAUNCHES 16
#define RTGS_ICP_STAMP_WGS 256
void rtgs_icp_set_stamps(void* dev);
/* TSDF integration (rtgs_slam.h, "meshing"): on != 0 selects the dense form, one thread per voxel over the whole grid with no
 * block test; 0 (default) the block-skipping form.  The planes are identical either way; the switch exists for A-B runs and
 * tests.  RTGS_TSDF_DENSE=1 at load time.  PROCESS-WIDE. */
void rtgs_tsdf_set_dense(int on);

#ifdef __cplusplus
}
#endif
#endif /* RTGS_DEBUG_H */
