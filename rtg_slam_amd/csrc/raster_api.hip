// C-ABI entry points of the rasterizer (include/rtgs_raster.h): argument checks, scratch-buffer
// carving, the rocPRIM scan / radix sort between the hand-written kernels, and launch order.
#include "../../include/rtgs_raster.h"
#include "../../include/rtgs_debug.h"
#include "raster_common.h"
#include "raster_launch.h"
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <math.h>
#include <new>
#include <stdlib.h>
#include <string.h>

// Everything a forward / backward remembers between calls lives in a context (include/rtgs_raster.h: rtgs_ctx).  The
// plain entry points use one process-wide default context; callers that render from several threads create one
// context per thread.
enum { EV_F0 = 0, EV_PRE, EV_SL_BIN, EV_SL_BLEND, EV_SCAN, EV_BIN0, EV_EMIT, EV_SORT, EV_RANGES, EV_BLEND0, EV_BLEND, EV_B0,
       EV_BWALK, EV_BBLEND, EV_BPRE, EV_N };
struct rtgs_ctx {
  int64_t stats[8] = {0};
  // The switches a context of the caller's own inherits from the default context (default_ctx() reads them from the
  // environment, rtgs_ctx_create copies the struct): a switch that belongs here is declared here and nowhere else.
  struct Switches {
    // Near-slice (occlusion) pass: 0 = off, 1 = always, 2 = automatic (large maps; the kernels themselves decide from
    // the depth histograms whether the slice is worth running - raster_common.h: slice_cut).
    int slice_mode = 2;
    int slice_budget = 384;
    int bwd_walk = 0;               // 0 / 3 = MFMA walk (default); 1 = strip walk everywhere; 2 = row-granular walk everywhere; 4 = per-tile choice between those two
    bool onepass = true;            // one-pass placement into per-tile segments where the layout provides them
    // Near slice: blend_fwd sorts each tile's list itself (lists of up to FSORT_CAP entries; RTGS_FWD_SORT=0: the sort
    // launches in front of it, as before).  With work counters set, the blend also leaves one word per tile - the class
    // its list took and its length - in `fsort_cls` (rtgs_raster_fused_sort_stats_ctx reduces them).
    bool fused_sort = true;
    bool speculation = true;        // the speculative forward (RTGS_FWD_SPECULATE; see rtgs_raster.h)
    bool plain_onepass = true;      // RTGS_PLAIN_ONEPASS=0: count / scan / scatter with the two host waits, as before round 6
    bool cull_cache = true, cull_check = false;   // the cull cache and its self-check (rtgs_raster_set_cull_cache_ctx)
    // Map step: the loss leaves one sign byte per pixel and the entry walk rebuilds the image gradients from it, where that
    // is possible (rtgs_raster_signs_ok_ctx); RTGS_LOSS_SIGNS=0: the float planes and slam_loss_grads' launch, as before.
    bool loss_signs = true;
    // Near slice of a speculative kind-1 forward: the blend's workgroups gather their own lists from row bands the shade
    // wrote, no bin_place (rtgs_debug.h: rtgs_raster_set_tile_gather_ctx).  0 off, 1 automatic, 2 forced (tests).
    int tile_gather = 1;
  } sw;
  int64_t gather_stats[4] = {0, 0, 0, 0};   // forwards that gathered; eligible ones that did not: listed / longest / layout
  // a gathered forward failed its guess over a list the blend's arena cannot sort: not again - forced mode included - until a
  // verified forward reports the longest slice list back inside the arena
  bool gather_blocked = false;
  int64_t loss_path_stats[2] = {0, 0};   // map steps whose backward read signs, map steps that took the float planes
  int64_t slice_stats[4] = {0};     // used, near-slice instances, tiles finished, tiles left to pass 2
  unsigned long long* counters = nullptr;
  uint32_t last_listed = 0;         // Gaussians the last verified speculative forward listed for binning
  uint32_t* fsort_cls = nullptr;    // device, [fsort_cap] words; 0xffffffff = the tile's workgroup did not get that far
  int32_t fsort_cap = 0, fsort_tiles = 0;
  bool prof = false;                // optional per-stage HIP-event timing (bench.py's roofline leg)
  bool force_sort_path = false;     // testing aid: take the global radix-sort binning path
  bool ev_init = false;
  hipEvent_t ev[EV_N];
  bool ev_set[EV_N] = {false};
  uint32_t* info_host = nullptr;    // pinned words the kernels publish totals into (the forward's host sync)
  uint32_t seq = 0;
  // what the most recent forward on this context left for its backward (see backward_impl)
  const void* hint_geom = nullptr;
  bool hint_slice_lists = true, hint_main_lists = true;
  int hint_walk = -2;               // what that forward wrote into tile_mode (-1 per-tile choice, 0 strip, 1 rows, 2 MFMA)
  void *last_geom = nullptr, *last_bin = nullptr, *last_img = nullptr;   // buffers of the most recent forward (rtgs_raster_last_buffers_ctx)
  uint32_t* aux_zero = nullptr;     // eight words the NEXT forward's blend clears (one-shot; rtgs_raster_set_aux_zero_ctx)
  // Automatic near-slice mode: whether a call takes the slice is decided on the device from that call's histograms and
  // never depends on history.  Only HOW the host learns it does: after a call that declined, the next one asks for the
  // decision (one extra pinned-flag sync, ~10 us) before it launches the slice's kernels instead of launching them
  // blind over an empty work list (~50 us of empty launches on a surface map).
  bool ask_first = false;
  // ---- speculative forward (RTGS_FWD_SPECULATE; see rtgs_raster.h) ----
  // What the last verified forward on this context looked like: the shape the next speculative one assumes.
  struct Plan {
    bool valid = false;
    int32_t P = 0, H = 0, W = 0;
    int kind = -1;                  // 0 = single pass, 1 = near slice finished every tile, 2 = slice declined, single pass over the visible list
    int slice_mode = 0, slice_budget = 0;
    uint32_t R = 0, R1 = 0, longest = 0, slots = 0, n_fin = 0;
    // slowly decaying maxima of the three totals: the capacities of the next speculative call come from these, so that
    // an optimisation that alternates between the views of a window (mapper.py:176-183 picks a random frame per
    // iteration) does not fail its guess every time it returns to the larger view
    uint32_t R_hi = 0, longest_hi = 0, slots_hi = 0;
    // ... and of the longest NEAR-SLICE tile list (slice_publish's payload word 1; per-tile segments only): what the tile
    // gather's eligibility looks at
    uint32_t slice_longest_hi = 0;
    void note_slice(uint32_t l) { slice_longest_hi = l > slice_longest_hi - slice_longest_hi / 16 ? l : slice_longest_hi - slice_longest_hi / 16; }
    void note(uint32_t r, uint32_t l, uint32_t s) {
      R = r; longest = l; slots = s;
      R_hi = r > R_hi - R_hi / 16 ? r : R_hi - R_hi / 16;
      longest_hi = l > longest_hi - longest_hi / 16 ? l : longest_hi - longest_hi / 16;
      slots_hi = s > slots_hi - slots_hi / 16 ? s : slots_hi - slots_hi / 16;
    }
  } plan;
  struct Spec {
    bool pending = false;           // a speculative forward awaits rtgs_raster_forward_verify
    int kind = -1;
    bool gathered = false;          // kind 1: the blend gathered its lists (tile_gather_chosen)
    uint32_t seq = 0, capR = 0, capL = 0, capS = 0;
    const void* geom = nullptr;     // geometry buffer of that forward (the backward guards itself only for this one)
    const uint32_t* fail_dev = nullptr;
    void* stream = nullptr;
    int32_t ntiles = 0;
    int64_t G_total = 0, B_total = 0, I_total = 0;
  } spec;
  int64_t spec_stats[3] = {0, 0, 0};   // speculative forwards, failed ones, forwards that could not speculate
  // Forwards WITHOUT a backward (the plain renders of a SLAM frame: RTGS_FWD_NO_BACKWARD) keep a history of their own - the
  // Gaussian count changes from one to the next, only the image and the sort class of the longest tile list are assumed -
  // and check their guess before they return (forward_speculative: `immediate`), so nothing is ever left pending.
  Plan plan_plain;                     // ... on large maps (the near slice is considered; kind 2 once it was declined)
  Plan plan_plain0;                    // ... on maps below the large-map size (kind 0: one pass over every Gaussian)
  int64_t plain_stats[2] = {0, 0};     // immediate one-pass forwards, those that had to be redone
  // ---- the cull cache (see rtgs_raster.h: rtgs_raster_set_cull_cache_ctx) ----
  // After a speculative forward of kind 1 or 2 ran the full cull and slice_hist, the per-row cull results in the geometry
  // buffer (radii, out_radii, tiles_touched, zbin, uv) and the three depth histograms are complete for `key`.  The next
  // such forward with an equal key launches recull_rows in their place: only the rows the map step's tail marked since
  // are recomputed.  EVERY other forward on the context disarms the cache.
  struct CullKey {
    const void *geom, *view, *means, *scales, *rots, *out_radii, *stream;
    uint64_t geom_bytes, epoch;
    int32_t P, H, W, kind, slice_mode, slice_budget;
    float fx, fy, cx, cy, tanfovx, tanfovy, scale_modifier, color_sigma;
  };
  struct CullCache {
    bool armed = false;
    CullKey key = {};
    uint8_t* marks = nullptr;          // inside the key's geometry buffer; what the tails write while the cache is armed
    uint64_t next_epoch = 0;           // one-shot, consumed by the next forward (0 = that forward may neither arm nor hit)
    int64_t stats[4] = {0, 0, 0, 0};   // hits, full culls that armed the cache, times an armed cache was dropped, view redos
    char* scratch = nullptr;           // self-check: a full cull's outputs
    size_t scratch_bytes = 0;
    unsigned long long* mismatches = nullptr;   // device word: differing words the self-check has seen
  } cull;
};

namespace rtgs {

static rtgs_ctx* default_ctx() {
  static rtgs_ctx* c = [] {
    rtgs_ctx* n = new rtgs_ctx();
    if (const char* e = getenv("RTGS_NEAR_SLICE")) n->sw.slice_mode = atoi(e);
    if (const char* e = getenv("RTGS_NEAR_SLICE_BUDGET")) { const int b = atoi(e); if (b > 0) n->sw.slice_budget = b; }
    if (const char* e = getenv("RTGS_SPECULATE")) n->sw.speculation = atoi(e) != 0;
    if (const char* e = getenv("RTGS_BIN_ONEPASS")) n->sw.onepass = atoi(e) != 0;
    if (const char* e = getenv("RTGS_FWD_SORT")) n->sw.fused_sort = atoi(e) != 0;
    if (const char* e = getenv("RTGS_PLAIN_ONEPASS")) n->sw.plain_onepass = atoi(e) != 0;
    if (const char* e = getenv("RTGS_BWD_WALK")) { const int m = atoi(e); n->sw.bwd_walk = (m >= 1 && m <= 4) ? m : 0; }
    if (const char* e = getenv("RTGS_CULL_CACHE")) n->sw.cull_cache = atoi(e) != 0;
    if (const char* e = getenv("RTGS_CULL_CACHE_CHECK")) n->sw.cull_check = atoi(e) != 0;
    if (const char* e = getenv("RTGS_LOSS_SIGNS")) n->sw.loss_signs = atoi(e) != 0;
    if (const char* e = getenv("RTGS_TILE_GATHER")) { const int m = atoi(e); n->sw.tile_gather = (m >= 0 && m <= 2) ? m : 1; }
    return n;
  }();
  return c;
}
static inline rtgs_ctx* use(rtgs_ctx* c) { return c ? c : default_ctx(); }

static void prof_mark(rtgs_ctx* c, int which, hipStream_t st) {
  if (!c->prof) return;
  if (!c->ev_init) {
    for (int i = 0; i < EV_N; ++i) (void)hipEventCreate(&c->ev[i]);
    c->ev_init = true;
  }
  (void)hipEventRecord(c->ev[which], st);
  c->ev_set[which] = true;
}

static int bits_for(uint32_t n) {   // bits needed to represent values in [0, n)
  int b = 0;
  while ((1ull << b) < (unsigned long long)n) ++b;
  return b < 1 ? 1 : b;
}

// The forward's host sync: spin on the pinned words a kernel publishes (raster_common.h: publish_to_host).  The payload is
// accepted only when the sequence word AND the checksum over (sequence, payload) agree with what was read: whatever order
// the device's writes become visible in, a torn view is re-read.  `pub` receives a consistent snapshot of the payload.
static int wait_published_words(uint32_t* info_host, uint32_t seq, hipStream_t st, uint32_t (&pub)[7]) {
  volatile uint32_t* h = info_host;
  auto snapshot_ok = [&]() -> bool {
    if (h[7] != seq) return false;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    uint32_t w[7];
    for (int k = 0; k < 7; ++k) w[k] = h[k];
    if (h[8] != host_checksum(seq, w)) return false;
    for (int k = 0; k < 7; ++k) pub[k] = w[k];
    return true;
  };
  for (long spin = 0; spin < 4000000L; ++spin) {
    if (snapshot_ok()) return RTGS_OK;
    __builtin_ia32_pause();
  }
  if (hipStreamSynchronize(st) != hipSuccess) return RTGS_E_HIP;   // the kernel has certainly finished: everything is visible now
  return snapshot_ok() ? RTGS_OK : RTGS_E_HIP;
}

// sort-class ceiling (launch_bin_tilesort) that covers lists of `longest` entries with a quarter of headroom
static uint32_t sort_class_cap(uint32_t longest) {
  const uint64_t want = (uint64_t)longest + longest / 4 + 16;
  const uint32_t classes[5] = {256u, 1024u, 3072u, 8192u, 16384u};
  for (uint32_t c : classes) if (want <= c) return c;
  return 16384u;
}

__global__ void bwd_info_kernel(BwdInfo* dst, SplatGrad* slot_grads, uint32_t slots, uint32_t use_slots) {
  dst->slot_grads = slot_grads; dst->slots = slots; dst->use_slots = use_slots;
}

// Maps of at least this many Gaussians (on >= 256 tiles) take the "large map" forward: the near slice is CONSIDERED (its
// kernels decide per call whether it runs) and tiles own segments for one-pass placement.  RTGS_LARGE_MAP_MIN at load time.
static int large_map_min() {
  static const int v = [] { const char* e = getenv("RTGS_LARGE_MAP_MIN"); const int x = e ? atoi(e) : 100000; return x > 0 ? x : 100000; }();
  return v;
}

// Offsets the BACKWARD reads (splats, radii, clamped, ranges1_bwd, list1) do not depend on `budget`: everything sized
// by the near-slice budget sits behind them, so a backward never needs to know the budget of its forward.
static GeomLayout geom_layout(int32_t P, int gx, int gy, int budget) {
  GeomLayout L{};
  size_t off = 0;
  const size_t Pn = (size_t)(P > 0 ? P : 1);
  L.splats = off; off = align_up(off + Pn * sizeof(Splat));
  L.tiles_touched = off; off = align_up(off + Pn * sizeof(uint32_t));
  L.offsets = off; off = align_up(off + Pn * sizeof(uint32_t));
  L.radii = off; off = align_up(off + Pn * sizeof(int32_t));
  L.clamped = off; off = align_up(off + Pn);
  L.sat = off; off = align_up(off + (size_t)(gx + 1) * (gy + 1) * sizeof(int32_t));
  {
    const size_t nt = (size_t)gx * gy;
    L.zero_begin = L.tile_count = off;           // tile_count .. slice_ctr are contiguous and cleared by preprocess_fwd
    off += nt * sizeof(uint32_t);                // (cursor / info / block_counts sit behind the zeroed span)
    L.tile_count1 = off; off += nt * sizeof(uint32_t);
    L.ranges1_bwd = off; off += nt * sizeof(uint2);
    L.slice_ctr = off; off += 8 * sizeof(uint32_t);   // [0] unfinished tiles [2] slice list length [3] cut [4] slot cursor of the slice, or visible-list length with [5] its slot cursor [6] speculation word [7] raised with it by recull_rows: the view moved
    L.slot_count = off; off += Pn * sizeof(uint32_t);   // zero between calls: cleared here, and again by grad_reduce
    L.zero_end = off; off = align_up(off);
    L.cursor = off; off = align_up(off + nt * sizeof(uint32_t));
    L.info = off; off = align_up(off + 4 * sizeof(uint32_t));
    L.block_counts = off; off = align_up(off + bin_block_counts_bytes((int)Pn, gx * gy));
    L.zbin = off; off = align_up(off + Pn);
    L.cursor1 = off; off = align_up(off + nt * sizeof(uint32_t));
    L.ranges1 = off; off = align_up(off + nt * sizeof(uint2));
    L.mask2 = off; off = align_up(off + nt * sizeof(int32_t));
    L.uv = off; off = align_up(off + Pn * sizeof(float2));
    // outside the zeroed span (see GeomLayout): the full cull clears the histograms through its second span
    L.slice_hist = off; off += 2 * SLICE_BINS * sizeof(uint32_t);
    L.slice_cover = off; off = align_up(off + SLICE_BINS * sizeof(unsigned long long));
    L.cull_marks = off; off = align_up(off + Pn + 16);
    L.cull_view = off; off = align_up(off + 16 * sizeof(float));
    L.slice_cap = nt * (size_t)(budget > 0 ? budget : 1);
    L.slice_max_list = L.slice_cap < 65536 ? L.slice_cap : 65536;   // every listed Gaussian covers >= 1 tile
    if (L.slice_max_list > Pn) L.slice_max_list = Pn;
    L.vis_ids = off; off = align_up(off + Pn * sizeof(uint32_t));             // work list of every visible Gaussian
    L.block_counts_vis = off; off = align_up(off + bin_list_block_counts_bytes((int)Pn, gx * gy));
    // one-pass placement (bin_place_kernel): on maps where the automatic mode considers the slice, every tile owns a
    // SEGMENT of SLICE_MAX_LIST entries in list1 / bucket1 (sparse use; 37 KB per tile, 119 MB at 1200x680 of 288 GB)
    L.slice_seg = (Pn >= (size_t)large_map_min() && nt >= 256) ? (size_t)SLICE_MAX_LIST : 0;
    const size_t cap1 = L.slice_seg ? (nt * L.slice_seg > L.slice_cap ? nt * L.slice_seg : L.slice_cap) : L.slice_cap;
    L.list1 = off; off = align_up(off + cap1 * sizeof(uint32_t));             // last budget-independent OFFSET
    L.block_counts1 = off; off = align_up(off + bin_slice_block_counts_bytes((int)Pn, L.slice_max_list, gx * gy));
    L.slice_ids = off; off = align_up(off + L.slice_max_list * sizeof(uint32_t));
    L.bucket1 = off; off = align_up(off + cap1 * sizeof(uint64_t));
  }
  size_t tb = 0, tb2 = 0;
  (void)rocprim::inclusive_scan(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, Pn, rocprim::plus<uint32_t>());
  (void)rocprim::exclusive_scan(nullptr, tb2, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, Pn, rocprim::plus<uint32_t>());
  if (tb2 > tb) tb = tb2;
  L.scan_temp_bytes = tb;
  L.scan_temp = off; off = align_up(off + tb);
  L.total = off;
  return L;
}

static BinLayout bin_layout(int64_t R, int ntiles, bool sort_path, size_t slots) {
  BinLayout L{};
  size_t off = 0;
  const size_t Rn = (size_t)(R > 0 ? R : 1);
  L.vals_b = off; off = align_up(off + Rn * sizeof(uint32_t));     // point_list: offset 0 in BOTH layouts
  L.keys_a = off; off = align_up(off + Rn * sizeof(uint64_t));     // tile buckets / unsorted keys
  if (!sort_path) {
    L.keys_b = L.vals_a = L.sort_temp = off; L.sort_temp_bytes = 0;
    if (slots > 0) { L.slot_grads = off; off = align_up(off + slots * sizeof(SplatGrad)); }   // BwdInfo
    L.total = off;
    return L;
  }
  L.keys_b = off; off = align_up(off + Rn * sizeof(uint64_t));
  L.vals_a = off; off = align_up(off + Rn * sizeof(uint32_t));
  size_t tb = 0;
  (void)rocprim::radix_sort_pairs(nullptr, tb, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                  (uint32_t*)nullptr, Rn, 0u, (unsigned)(32 + bits_for((uint32_t)ntiles)));
  L.sort_temp_bytes = tb;
  L.sort_temp = off; off = align_up(off + tb);
  L.total = off;
  return L;
}

static ImgLayout img_layout(int H, int W, int ntiles) {
  ImgLayout L{};
  size_t off = 0;
  L.ranges = off; off = align_up(off + (size_t)ntiles * sizeof(uint2));
  L.n_contrib = off; off = align_up(off + (size_t)H * W * sizeof(uint32_t));
  L.bwd_info = off; off = align_up(off + sizeof(BwdInfo));
  L.tile_mode = off; off = align_up(off + (size_t)ntiles * sizeof(uint32_t));
  L.depth_pos = off; off = align_up(off + (size_t)H * W * sizeof(uint32_t));
  L.tile_last = off; off = align_up(off + (size_t)ntiles * sizeof(uint32_t));
  // the TileCache (raster_common.h): 48 B of record + 2 B of block mask for the first TILE_RECS list positions of every tile
  // (39.6 + 1.7 MB at 1200x680), two plane words per pixel
  L.tile_recs = off; off = align_up(off + (size_t)ntiles * TILE_RECS * 3 * sizeof(float4));
  L.tile_masks = off; off = align_up(off + (size_t)ntiles * TILE_RECS * sizeof(uint16_t));
  L.depth_aux = off; off = align_up(off + (size_t)H * W * sizeof(float2));
  L.total = off;
  return L;
}

static int make_params(const rtgs_raster_settings* s, int32_t P, int32_t M, RasterParams& p) {
  if (!s || P < 0 || M < 1 || M > 16) return RTGS_E_INVALID;
  if (s->image_height <= 0 || s->image_width <= 0) return RTGS_E_INVALID;
  if (s->sh_degree < 0 || s->sh_degree > 3 || (s->sh_degree + 1) * (s->sh_degree + 1) > M) return RTGS_E_INVALID;
  if (!s->bg || !s->viewmatrix || !s->campos) return RTGS_E_INVALID;
  p.H = s->image_height; p.W = s->image_width;
  p.gx = (p.W + TILE - 1) / TILE; p.gy = (p.H + TILE - 1) / TILE;
  p.P = P; p.M = M; p.deg = s->sh_degree;
  p.tanfovx = s->tanfovx; p.tanfovy = s->tanfovy;
  p.fx = (float)(p.W / (2.0 * (double)s->tanfovx));      // utils/graphics_utils.py:89-90
  p.fy = (float)(p.H / (2.0 * (double)s->tanfovy));
  p.cx = s->cx > 0.f ? s->cx : 0.5f * (float)(p.W - 1);
  p.cy = s->cy > 0.f ? s->cy : 0.5f * (float)(p.H - 1);
  p.scale_modifier = s->scale_modifier;
  p.opaque_thr = s->opaque_threshold; p.depth_thr = s->depth_threshold; p.normal_thr = s->normal_threshold;
  p.color_sigma = s->color_sigma; p.T_thr = s->T_threshold;
  p.view = s->viewmatrix; p.campos = s->campos; p.bg = s->bg;
  p.spec_fail = nullptr;
  return RTGS_OK;
}

#define HIP_TRY(expr)                         \
  do {                                        \
    hipError_t e_ = (expr);                   \
    if (e_ != hipSuccess) return RTGS_E_HIP;  \
  } while (0)

static int dbg_sync(const rtgs_raster_settings* s, hipStream_t st) {
  if (s->debug) {
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
  }
  return RTGS_OK;
}
#define DBG(s, st)                              \
  do {                                          \
    int r_ = dbg_sync(s, st);                   \
    if (r_ != RTGS_OK) return r_;               \
  } while (0)

// ---- the forward's host side: one per-call struct, one function per stage (rtgs_raster_forward_ctx is the driver) -------
// What one forward works with.  Built once on the entry point's stack and handed to the stage functions by reference.
struct FwdCall {
  rtgs_ctx* c;
  const rtgs_raster_settings* s;
  RasterParams p;
  hipStream_t st;
  int32_t flags;
  bool want_bwd, slice_auto;
  // the caller's arrays, outputs and resize callbacks
  const float *means3D, *opacities, *shs, *scales, *rotations, *normal_w;
  const int32_t* tile_mask;
  float *out_color, *out_depth, *out_cw, *out_dw, *out_T;
  int32_t *out_cidx, *out_didx, *out_radii;
  rtgs_resize_fn geom_resize, binning_resize, image_resize;
  void *geom_user, *binning_user, *image_user;
  int64_t* num_rendered_host;
  // the geometry and image buffers, and typed pointers into them
  GeomLayout G;
  ImgLayout I;
  char *geom, *img;
  uint32_t *tiles_touched, *offsets, *tile_count, *cursor, *info, *zero_words, *tile_count1, *slice_hist, *slice_ctr, *list1;
  Splat* splats; int32_t *radii, *sat, *mask2; uint8_t *clamped, *zbin; uint16_t* block_counts;
  uint2 *ranges, *ranges1, *ranges1_bwd; unsigned long long* slice_cover; float2* uv;
  // tile_mode is always written, also under RTGS_FWD_NO_BACKWARD: a backward that is called anyway (slower, atomics) must
  // not meet stale walk choices of an earlier forward in a recycled image buffer
  uint32_t *n_contrib, *depth_pos, *tile_last, *tile_mode;
  int zero_n, ntiles;
  int fwd_walk;           // what blend_fwd writes into tile_mode: MFMA walk 2 (default), forced strip 0 / rows 1, per-tile choice -1
  TileCache tcache;       // what blend_fwd leaves for the entry-per-lane backward (nothing when there is no backward)
  uint32_t seg1;          // one-pass placement of the near slice's instances into per-tile segments (0: count / scan / scatter)
  uint32_t* aux_zero;     // the context's one-shot state, consumed by this call: these words, and the cull cache's
  uint64_t cull_epoch;
  bool cull_was_armed;
  // pinned host words the kernels publish totals into (a spin of a few microseconds instead of the ~25 us a blocking
  // hipStreamSynchronize takes to wake up; bounded, falls back), and the last consistent snapshot of them
  uint32_t* info_host;
  uint32_t pub[7];
};

static inline void next_seq(rtgs_ctx* c) { if (++c->seq == 0u) c->seq = 1u; }
static inline int wait_published(FwdCall& f) { return wait_published_words(f.info_host, f.c->seq, f.st, f.pub); }

static void record_stats(rtgs_ctx* c, int64_t rendered, int ntiles, int64_t geom_bytes, int64_t bin_bytes, int64_t img_bytes,
                         bool tile_path, int64_t longest) {
  c->stats[0] = rendered; c->stats[1] = 32 + bits_for((uint32_t)ntiles); c->stats[2] = ntiles;
  c->stats[3] = geom_bytes; c->stats[4] = bin_bytes; c->stats[5] = img_bytes;
  c->stats[6] = tile_path ? 1 : 0; c->stats[7] = longest;
}

// What the next forward on this context may assume, from the FINAL state of a classic one: `kind` < 0 leaves no plan.  The
// decaying maxima start over on another image (`same`: and, for the map step's plan, another Gaussian count).
static void note_plan(rtgs_ctx::Plan& pl, const FwdCall& f, bool same, int kind, bool usable, int64_t R, uint32_t longest,
                      uint32_t slots) {
  same = same && pl.valid && pl.H == f.p.H && pl.W == f.p.W;
  pl.kind = kind;
  pl.valid = kind >= 0 && usable && R <= 0xffffffffll;
  pl.P = f.p.P; pl.H = f.p.H; pl.W = f.p.W; pl.slice_mode = f.c->sw.slice_mode; pl.slice_budget = f.c->sw.slice_budget;
  if (!same || !pl.valid) { pl.R_hi = pl.longest_hi = pl.slots_hi = 0; pl.slice_longest_hi = 0; }
  pl.note((uint32_t)R, longest, slots);
}

// The near slice's selection: depth bins up to the cut the kernels derive from this call's histograms.
static SliceSel slice_sel(const FwdCall& f) {
  return SliceSel{1, f.zbin, f.slice_hist, (uint32_t)f.G.slice_cap, (uint32_t)f.G.slice_max_list, f.slice_ctr, nullptr, nullptr,
                  f.slice_cover, (uint32_t)f.ntiles * (uint32_t)(TILE * TILE), f.slice_auto ? 1 : 0};
}

// Launch wrappers that fill in the call's arrays (`p`: the call's parameters, or their guarded copy).
static void preprocess_all(const FwdCall& f, const int32_t* sat, bool clear) {
  launch_preprocess_fwd(f.p, f.means3D, f.opacities, f.shs, f.scales, f.rotations, f.normal_w, sat, f.splats, f.tiles_touched,
                        f.radii, f.clamped, f.out_radii, clear ? f.zero_words : nullptr, clear ? f.zero_n : 0, nullptr, f.st);
}
static void shade(const FwdCall& f, const RasterParams& p, SliceList work, const SliceSel& sel, size_t max_list,
                  RowBands rb = RowBands{nullptr, nullptr, 0u}) {
  launch_preprocess_shade(p, f.means3D, f.opacities, f.shs, f.scales, f.rotations, f.normal_w, f.splats, f.radii, f.clamped,
                          f.uv, work, sel, max_list, f.st, rb);
}
static void blend(const FwdCall& f, const RasterParams& p, const uint2* ranges, const uint32_t* list, SlicePass pass,
                  uint32_t seg, FusedSort fs = FusedSort{nullptr, nullptr, nullptr, nullptr, nullptr},
                  TileGather tg = TileGather{nullptr, nullptr, 0u, nullptr, nullptr, nullptr}) {
  launch_blend_fwd(p, ranges, list, f.splats, f.out_color, f.out_depth, f.out_cidx, f.out_didx, f.out_cw, f.out_dw, f.out_T,
                   f.n_contrib, f.c->counters, pass, f.tile_mode, f.depth_pos, f.tile_last, f.fwd_walk, f.aux_zero, f.tcache,
                   seg, f.st, fs, tg);
}

// The tile gather (Switches::tile_gather): may this speculative kind-1 forward leave bin_place and the long-list sort launch
// out?  The structure must be the one the gather stands on - per-tile segments, the fused sort - and the layout must hold
// the bands: entries are x0 | x1 << 8 | list position << 16, the shade counts rows in LDS, and gy bands of max_list words
// must fit the bucket nobody else uses on this path.  Then, from the last verified forwards and without a host wait: the
// work list within max_list, and the decayed longest slice list at most 7/8 of what the blend's arena sorts.  Forced mode
// looks at neither.  In both modes a gathered forward that failed over a list above the arena blocks the path
// (rtgs_raster_forward_verify_ctx); the classic call that redoes the step reports that list (forward_classic: note_slice),
// and the path stays off for as long as the reported maximum stays above the arena: no alternation between gather and redo.
static bool tile_gather_chosen(FwdCall& f, const rtgs_ctx::Plan& pl) {
  rtgs_ctx* const c = f.c; const GeomLayout& G = f.G;
  if (c->sw.tile_gather == 0 || !f.seg1 || !(c->sw.fused_sort && blend_fwd_fuses_sort() && blend_fwd_gathers())) return false;
  const size_t cap1 = (size_t)f.ntiles * G.slice_seg > G.slice_cap ? (size_t)f.ntiles * G.slice_seg : G.slice_cap;
  if (f.p.gx > 255 || f.p.gy > GATHER_ROWS_MAX || G.slice_max_list > 65536 ||
      (size_t)f.p.gy * G.slice_max_list * sizeof(uint32_t) > cap1 * sizeof(uint64_t)) { ++c->gather_stats[3]; return false; }
  const bool forced = c->sw.tile_gather == 2;
  if (c->gather_blocked && pl.slice_longest_hi <= (uint32_t)FSORT_CAP) c->gather_blocked = false;
  if (c->gather_blocked) { ++c->gather_stats[2]; return false; }
  if (!forced && c->last_listed > (uint32_t)G.slice_max_list) { ++c->gather_stats[1]; return false; }
  if (!forced && pl.slice_longest_hi > (uint32_t)(FSORT_CAP - FSORT_CAP / 8)) { ++c->gather_stats[2]; return false; }
  ++c->gather_stats[0];
  return true;
}

// gradient slots of the backward (BwdInfo): gbase = exclusive scan of the rect areas, into `offsets`
static int scan_slots(const FwdCall& f) {
  size_t tb = f.G.scan_temp_bytes;
  HIP_TRY(rocprim::exclusive_scan(f.geom + f.G.scan_temp, tb, f.tiles_touched, f.offsets, 0u, (size_t)f.p.P,
                                  rocprim::plus<uint32_t>(), f.st));
  return RTGS_OK;
}

// The near slice's tile lists, after their placement into bucket1: sorted by the sort launches into list1, or - fused -
// by the blend's own workgroups (fs1 tells it where the keys are); then only the size class that does not fit the
// blend's LDS keeps its launch.  (That launch is unconditional: a slice whose longest list fits the blend still pays it.)
// (with work counters set: the per-tile class words of the fused blend, cleared; nullptr otherwise)
static int fsort_class_words(FwdCall& f, uint32_t*& cls) {
  rtgs_ctx* const c = f.c;
  cls = nullptr;
  if (c->counters) {
    if (c->fsort_cap < f.ntiles) {
      if (c->fsort_cls) (void)hipFree(c->fsort_cls);
      c->fsort_cls = nullptr; c->fsort_cap = 0;
      HIP_TRY(hipMalloc((void**)&c->fsort_cls, (size_t)f.ntiles * sizeof(uint32_t)));
      c->fsort_cap = f.ntiles;
    }
    HIP_TRY(hipMemsetAsync(c->fsort_cls, 0xff, (size_t)f.ntiles * sizeof(uint32_t), f.st));
    c->fsort_tiles = f.ntiles;
    cls = c->fsort_cls;
  }
  return RTGS_OK;
}
static int sort_slice_lists(FwdCall& f, FusedSort& fs1) {
  rtgs_ctx* const c = f.c;
  const unsigned long long* bucket1 = (const unsigned long long*)(f.geom + f.G.bucket1);
  const uint32_t* cnt = f.seg1 ? f.tile_count1 : nullptr;
  if (!(c->sw.fused_sort && blend_fwd_fuses_sort())) {
    launch_bin_tilesort(f.ntiles, (uint32_t)SLICE_MAX_LIST, f.ranges1, bucket1, f.list1, nullptr, f.st, cnt, f.seg1,
                        f.seg1 ? f.ranges1 : nullptr);
    return RTGS_OK;
  }
  launch_bin_tilesort_long(f.ntiles, f.ranges1, bucket1, f.list1, nullptr, f.st, cnt, f.seg1);
  uint32_t* cls = nullptr;
  const int rc = fsort_class_words(f, cls);
  if (rc != RTGS_OK) return rc;
  fs1 = FusedSort{bucket1, cnt, f.seg1 ? f.ranges1 : nullptr, f.list1, cls};
  return RTGS_OK;
}

// Pass 1 over the slice's work list (slice_compact laid it out): shade, bin, sort and blend only the nearest Gaussians, then
// publish how many tiles are left.  No host sync: the arrays are sized by the budget, the sort classes are launched blind.
// The caller has advanced c->seq; `guard` is the speculation word slice_publish raises (nullptr: nothing is guessed).
static int slice_pass1(FwdCall& f, uint32_t* guard, bool gather = false) {
  const RasterParams& p = f.p; const GeomLayout& G = f.G;
  const SliceSel sel1 = slice_sel(f);
  const SliceList work{(const uint32_t*)(f.geom + G.slice_ids), f.slice_ctr + 2};
  unsigned long long* const bucket1 = (unsigned long long*)(f.geom + G.bucket1);
  if (gather) {
    // The tile gather: the shade leaves row bands in the bucket (their counters: the main pass' tile counters, which the cull
    // stage cleared and a kind-1 forward never uses), the blend's workgroups build, sort and count their own lists.  No
    // bin_place, no sort launch; the blend writes tile_count1 and ranges1 as they did.
    const RowBands rb{f.tile_count, (uint32_t*)bucket1, (uint32_t)G.slice_max_list};
    shade(f, p, work, sel1, G.slice_max_list, rb);
    uint32_t* cls = nullptr;
    const int rcc = fsort_class_words(f, cls);
    if (rcc != RTGS_OK) return rcc;
    DBG(f.s, f.st);
    prof_mark(f.c, EV_SL_BIN, f.st);
    blend(f, p, f.ranges1, f.list1, SlicePass{1, f.tile_mask, f.mask2, f.ranges1_bwd, f.ranges}, f.seg1,
          FusedSort{bucket1, f.tile_count1, f.ranges1, f.list1, cls},
          TileGather{rb.count, rb.entries, rb.stride, work.ids, f.radii, f.tile_count1});
    prof_mark(f.c, EV_SL_BLEND, f.st);
    launch_slice_publish(f.ntiles, f.tile_mask, f.mask2, f.info + 2, f.slice_ctr, f.info_host, f.c->seq, guard, f.st, f.tile_count1);
    DBG(f.s, f.st);
    return RTGS_OK;
  }
  shade(f, p, work, sel1, G.slice_max_list);
  if (f.seg1) {       // one pass: no count, no scan (tile_count1 was cleared by the cull pass; the sort writes ranges1)
    launch_bin_place(p, f.splats, f.radii, f.tile_mask, f.tile_count1, bucket1, f.seg1, nullptr, sel1, work, G.slice_max_list, f.st);
  } else {
    uint16_t* const block_counts1 = (uint16_t*)(f.geom + G.block_counts1);
    uint32_t* const cursor1 = (uint32_t*)(f.geom + G.cursor1);
    if (launch_bin_count(p, f.splats, f.radii, f.tile_mask, f.tile_count1, block_counts1, sel1, work, G.slice_max_list, f.st) != 0)
      return RTGS_E_HIP;
    launch_bin_tilescan(f.ntiles, f.tile_count1, f.ranges1, cursor1, f.info + 2, nullptr, nullptr, nullptr, nullptr, nullptr, 0u,
                        SpecCaps{nullptr, 0u, 0u, 0u, nullptr}, f.st);
    launch_bin_scatter(p, f.splats, f.radii, f.tile_mask, block_counts1, cursor1, bucket1, sel1, work, G.slice_max_list, f.st);
  }
  FusedSort fs1{nullptr, nullptr, nullptr, nullptr, nullptr};
  const int rc = sort_slice_lists(f, fs1);
  if (rc != RTGS_OK) return rc;
  DBG(f.s, f.st);
  prof_mark(f.c, EV_SL_BIN, f.st);
  blend(f, p, f.ranges1, f.list1, SlicePass{1, f.tile_mask, f.mask2, f.ranges1_bwd, f.ranges}, f.seg1, fs1);
  prof_mark(f.c, EV_SL_BLEND, f.st);      // the bracket holds the blend alone (bench.py's roofline divides by it)
  launch_slice_publish(f.ntiles, f.tile_mask, f.mask2, f.info + 2, f.slice_ctr, f.info_host, f.c->seq, guard, f.st,
                       f.seg1 ? f.tile_count1 : nullptr);
  DBG(f.s, f.st);
  return RTGS_OK;
}

// The cull cache's self-check on a hit: a full cull and slice_hist into scratch copies, compared word for word on the
// device (uv of a culled row is not written by the cull: the scratch starts from the maintained array).
static int cull_self_check(FwdCall& f, uint32_t* fail) {
  rtgs_ctx::CullCache& cc = f.c->cull;
  const int32_t P = f.p.P; const size_t Pn = (size_t)P;
  const size_t o_tt = 0, o_rad = align_up(o_tt + Pn * 4), o_orad = align_up(o_rad + Pn * 4), o_zb = align_up(o_orad + Pn * 4),
               o_uv = align_up(o_zb + Pn), o_hist = align_up(o_uv + Pn * 8), need = align_up(o_hist + CULL_HIST_WORDS * 4);
  if (cc.scratch_bytes < need) {
    if (cc.scratch) (void)hipFree(cc.scratch);
    cc.scratch = nullptr; cc.scratch_bytes = 0;
    HIP_TRY(hipMalloc((void**)&cc.scratch, need));
    cc.scratch_bytes = need;
  }
  if (!cc.mismatches) {
    HIP_TRY(hipMalloc((void**)&cc.mismatches, sizeof(unsigned long long)));
    HIP_TRY(hipMemset(cc.mismatches, 0, sizeof(unsigned long long)));
  }
  char* sc = cc.scratch;
  HIP_TRY(hipMemcpyAsync(sc + o_uv, f.uv, Pn * 8, hipMemcpyDeviceToDevice, f.st));
  launch_preprocess_cull(f.p, f.means3D, f.scales, f.rotations, (uint32_t*)(sc + o_tt), (int32_t*)(sc + o_rad),
                         f.out_radii ? (int32_t*)(sc + o_orad) : nullptr, nullptr, 0, (uint8_t*)(sc + o_zb),
                         (float2*)(sc + o_uv), (uint32_t*)(sc + o_hist), f.st);
  launch_slice_hist(P, (const uint8_t*)(sc + o_zb), (const uint32_t*)(sc + o_tt), (const int32_t*)(sc + o_rad),
                    (uint32_t*)(sc + o_hist), (unsigned long long*)(sc + o_hist + 2 * SLICE_BINS * 4), f.st);
  launch_cull_check(P, f.tiles_touched, (const uint32_t*)(sc + o_tt), f.radii, (const int32_t*)(sc + o_rad), f.out_radii,
                    (const int32_t*)(sc + o_orad), f.zbin, (const uint8_t*)(sc + o_zb), f.uv, (const float2*)(sc + o_uv),
                    f.slice_hist, (const uint32_t*)(sc + o_hist), fail + 1, cc.mismatches, f.st);
  return RTGS_OK;
}

// The geometry of every Gaussian and the depth histograms, for a speculative forward of `kind` 1 or 2: the cull (MODE 1) and
// slice_hist over the whole map - or, when the cache holds both for exactly this call, recull_rows over the rows the last
// tail marked.  Only a forward that may use the cache (`usable`) arms it again.
static int cull_stage(FwdCall& f, int kind, bool usable, uint32_t* fail, const BwdInfoInit& bi) {
  rtgs_ctx* const c = f.c; const RasterParams& p = f.p;
  rtgs_ctx::CullCache& cc = c->cull;
  rtgs_ctx::CullKey key;
  memset(&key, 0, sizeof(key));
  key.geom = f.geom; key.view = f.s->viewmatrix; key.means = f.means3D; key.scales = f.scales; key.rots = f.rotations;
  key.out_radii = f.out_radii; key.stream = (void*)f.st; key.geom_bytes = (uint64_t)f.G.total; key.epoch = f.cull_epoch;
  key.P = p.P; key.H = p.H; key.W = p.W; key.kind = kind; key.slice_mode = c->sw.slice_mode; key.slice_budget = c->sw.slice_budget;
  key.fx = p.fx; key.fy = p.fy; key.cx = p.cx; key.cy = p.cy; key.tanfovx = p.tanfovx; key.tanfovy = p.tanfovy;
  key.scale_modifier = p.scale_modifier; key.color_sigma = p.color_sigma;
  usable = usable && c->sw.cull_cache && f.cull_epoch != 0;
  uint8_t* const marks = (uint8_t*)(f.geom + f.G.cull_marks);
  float* const view_copy = (float*)(f.geom + f.G.cull_view);
  if (usable && f.cull_was_armed && memcmp(&key, &cc.key, sizeof(key)) == 0) {
    launch_recull_rows(p, f.means3D, f.scales, f.rotations, f.tiles_touched, f.radii, f.out_radii, f.zero_words, f.zero_n, f.zbin,
                       f.uv, f.slice_hist, f.slice_cover, marks, view_copy, (int)(fail - f.zero_words), bi, f.st);
    cc.armed = true;
    ++cc.stats[0]; --cc.stats[2];
    return c->sw.cull_check ? cull_self_check(f, fail) : RTGS_OK;
  }
  launch_preprocess_cull(p, f.means3D, f.scales, f.rotations, f.tiles_touched, f.radii, f.out_radii, f.zero_words, f.zero_n,
                         f.zbin, f.uv, f.slice_hist, f.st);
  launch_slice_hist(p.P, f.zbin, f.tiles_touched, f.radii, f.slice_hist, f.slice_cover, f.st, bi);
  if (usable) {
    // the arrays are complete for this key from here on: no stale marks, and the view they were computed with
    HIP_TRY(hipMemsetAsync(marks, 0, align_up((size_t)p.P + 16), f.st));
    HIP_TRY(hipMemcpyAsync(view_copy, f.s->viewmatrix, 16 * sizeof(float), hipMemcpyDeviceToDevice, f.st));
    memcpy(&cc.key, &key, sizeof(key)); cc.marks = marks; cc.armed = true;
    ++cc.stats[1];
  }
  return RTGS_OK;
}

// The buffers of the call - resize callbacks: geometry, then image; the binning buffer is sized later, by the path that is
// taken - and everything derived from them and from the context's switches.
static int forward_setup(FwdCall& f) {
  rtgs_ctx* const c = f.c;
  const RasterParams& p = f.p;
  f.ntiles = p.gx * p.gy;
  f.G = geom_layout(p.P, p.gx, p.gy, c->sw.slice_budget);
  f.geom = (char*)f.geom_resize(f.geom_user, f.G.total);
  f.I = img_layout(p.H, p.W, f.ntiles);
  f.img = (char*)f.image_resize(f.image_user, f.I.total);
  if (!f.geom || !f.img) return RTGS_E_ALLOC;
  const GeomLayout& G = f.G;
  const ImgLayout& I = f.I;
  char *const geom = f.geom, *const img = f.img;
  c->last_geom = geom; c->last_img = img; c->last_bin = nullptr;
  for (int i = 0; i < EV_B0; ++i) c->ev_set[i] = false;
  prof_mark(c, EV_F0, f.st);
  f.splats = (Splat*)(geom + G.splats); f.tiles_touched = (uint32_t*)(geom + G.tiles_touched); f.offsets = (uint32_t*)(geom + G.offsets);
  f.radii = (int32_t*)(geom + G.radii); f.clamped = (uint8_t*)(geom + G.clamped); f.sat = (int32_t*)(geom + G.sat);
  f.tile_count = (uint32_t*)(geom + G.tile_count); f.cursor = (uint32_t*)(geom + G.cursor); f.info = (uint32_t*)(geom + G.info);
  f.block_counts = (uint16_t*)(geom + G.block_counts);
  f.zero_words = (uint32_t*)(geom + G.zero_begin); f.zero_n = (int)((G.zero_end - G.zero_begin) / sizeof(uint32_t));
  f.tile_count1 = (uint32_t*)(geom + G.tile_count1); f.ranges1 = (uint2*)(geom + G.ranges1); f.ranges1_bwd = (uint2*)(geom + G.ranges1_bwd);
  f.slice_hist = (uint32_t*)(geom + G.slice_hist); f.slice_cover = (unsigned long long*)(geom + G.slice_cover);
  f.slice_ctr = (uint32_t*)(geom + G.slice_ctr); f.zbin = (uint8_t*)(geom + G.zbin); f.mask2 = (int32_t*)(geom + G.mask2);
  f.list1 = (uint32_t*)(geom + G.list1); f.uv = (float2*)(geom + G.uv);
  f.ranges = (uint2*)(img + I.ranges); f.n_contrib = (uint32_t*)(img + I.n_contrib); f.depth_pos = (uint32_t*)(img + I.depth_pos);
  f.tile_last = (uint32_t*)(img + I.tile_last); f.tile_mode = (uint32_t*)(img + I.tile_mode);
  f.tcache = f.want_bwd ? TileCache{(float4*)(img + I.tile_recs), (uint16_t*)(img + I.tile_masks), (float2*)(img + I.depth_aux)}
                        : TileCache{nullptr, nullptr, nullptr};
  f.fwd_walk = c->sw.bwd_walk == 0 || c->sw.bwd_walk == 3 ? 2 : (c->sw.bwd_walk == 4 ? -1 : c->sw.bwd_walk - 1);
  f.seg1 = c->sw.onepass ? (uint32_t)G.slice_seg : 0u;      // RTGS_BIN_ONEPASS=0: count / scan / scatter
  f.slice_auto = c->sw.slice_mode == 2;
  if (!c->info_host) {
    HIP_TRY(hipHostMalloc((void**)&c->info_host, HOST_WORDS * sizeof(uint32_t), hipHostMallocCoherent));
    memset(c->info_host, 0, HOST_WORDS * sizeof(uint32_t));
  }
  f.info_host = c->info_host;
  for (uint32_t& w : f.pub) w = 0;
  return RTGS_OK;
}

// Speculative forward (RTGS_FWD_SPECULATE): no host wait inside the call.  The host assumes the call looks like the last
// verified one on this context - same kind of pass structure, instance / list / slot totals within a margin of the last
// ones - sizes the binning buffer and picks the sort classes from that, and enqueues EVERYTHING; the kernel that learns
// the real numbers (bin_tilescan, or slice_publish) checks them against the capacities and raises a device word if they
// do not hold, on which every later kernel that could overrun a buffer or touch persistent state returns at once.
// rtgs_raster_forward_verify reads the published numbers afterwards (the GPU is busy with the rest of the step by
// then) and tells the caller whether to redo the step without speculation.  Results are those of the plain call.
//
// `immediate`: a forward without a backward whose last such forward on this image declined the near slice runs the same
// one-pass flow (no count / scan / scatter, no host wait before the blend) and looks at the published totals itself,
// while the blend runs; a wrong guess (a list outgrew the assumed sort class, the slice was taken after all) goes on to
// the classic path.  Nothing but the image size and that class is assumed: P may differ.
//
// RETURNED: the call is over, the return value is its result (an error, a pending guess, a checked immediate one);
// NOT_ELIGIBLE: nothing was launched; REDO: the immediate guess did not hold, go on classically
enum SpecOutcome { SPEC_RETURNED, SPEC_NOT_ELIGIBLE, SPEC_REDO };

static int forward_speculative(FwdCall& f, bool sort_path, bool sliced, SpecOutcome& outcome) {
  rtgs_ctx* const c = f.c;
  const RasterParams& p = f.p; const GeomLayout& G = f.G; const ImgLayout& I = f.I;
  const int32_t P = p.P; const int ntiles = f.ntiles; hipStream_t st = f.st;
  int rc;
  outcome = SPEC_RETURNED;
  rtgs_ctx::Plan& pp = sliced ? c->plan_plain : c->plan_plain0;
  const bool immediate = !(f.flags & RTGS_FWD_SPECULATE) && !f.want_bwd && c->sw.speculation && c->sw.plain_onepass && c->sw.onepass &&
                         P > 0 && !sort_path && !f.s->debug && pp.valid && (sliced ? (pp.kind == 2 && G.slice_seg) : pp.kind == 0) &&
                         pp.H == p.H && pp.W == p.W && pp.slice_mode == c->sw.slice_mode && pp.slice_budget == c->sw.slice_budget;
  const rtgs_ctx::Plan& pl = immediate ? pp : c->plan;
  const bool eligible = immediate ||
                        ((f.flags & RTGS_FWD_SPECULATE) && c->sw.speculation && f.want_bwd && P > 0 && !sort_path && !f.s->debug &&
                         pl.valid && pl.P == P && pl.H == p.H && pl.W == p.W && pl.slice_mode == c->sw.slice_mode &&
                         pl.slice_budget == c->sw.slice_budget && (pl.kind == 0 ? !sliced : (pl.kind == 1 || pl.kind == 2) && sliced));
  const uint32_t capR = pl.R_hi + pl.R_hi / 8u + 8192u, capL = sort_class_cap(pl.longest_hi),
                 capS = immediate ? 0u : pl.slots_hi + pl.slots_hi / 8u + 8192u;
  if (!(eligible && (pl.kind == 1 || capS <= SLOTS_MAX))) {
    if (f.flags & RTGS_FWD_SPECULATE) ++c->spec_stats[2];
    outcome = SPEC_NOT_ELIGIBLE;
    return RTGS_OK;
  }
  uint32_t* const fail = f.slice_ctr + 6;            // inside the span every forward clears
  next_seq(c);
  // Kind 1, the near slice finished every tile last time: pass 1 only, the slot space is the slice's instance budget.
  // Kinds 0 and 2: one pass (kind 2: through the visible list); with `seg2` every tile owns a segment of the sort class that
  // covered the last verified longest list, and a list that outgrows it raises `fail` like any other wrong guess (a forward
  // without a backward on a small map - `immediate`, kind 0 - takes segments too: no count, no scan).
  const uint32_t sl = (uint32_t)G.slice_cap <= SLOTS_MAX ? (uint32_t)G.slice_cap : 0u;
  const uint32_t seg2 = (pl.kind != 1 && c->sw.onepass && ((pl.kind == 2 && G.slice_seg) || (immediate && pl.kind == 0))) ? capL : 0u;
  const bool seg_main = seg2 != 0u;          // main pass placed into per-tile segments: no bound on the total
  const BinLayout B = pl.kind == 1 ? bin_layout(0, ntiles, false, (size_t)sl)
                                   : bin_layout(seg2 ? (int64_t)ntiles * (int64_t)seg2 : (int64_t)capR, ntiles, false, (size_t)capS);
  char* bin = (char*)f.binning_resize(f.binning_user, B.total);
  if (!bin) return RTGS_E_ALLOC;
  c->last_bin = bin;
  BwdInfo* const bwd_info = (BwdInfo*)(f.img + I.bwd_info);
  SplatGrad* const slot_grads = (SplatGrad*)(bin + B.slot_grads);
  if (pl.kind == 1) {
    if ((rc = cull_stage(f, pl.kind, !immediate, fail, BwdInfoInit{bwd_info, slot_grads, sl, sl ? 1u : 0u})) != RTGS_OK) return rc;
    prof_mark(c, EV_PRE, st);
    launch_slice_compact(P, slice_sel(f), (uint32_t*)(f.geom + G.slice_ids), f.slice_ctr + 2, f.tiles_touched, f.offsets,
                         f.slice_ctr + 4, nullptr, 0u, nullptr, st);
    c->spec.gathered = tile_gather_chosen(f, pl);
    if ((rc = slice_pass1(f, fail, c->spec.gathered)) != RTGS_OK) return rc;
    prof_mark(c, EV_BLEND0, st); prof_mark(c, EV_BLEND, st);
    c->hint_slice_lists = true; c->hint_main_lists = false;
    c->slice_stats[0] = 1; c->slice_stats[1] = pl.R1; c->slice_stats[2] = pl.n_fin; c->slice_stats[3] = 0;
  } else {
    unsigned long long* const keys_a = (unsigned long long*)(bin + B.keys_a);
    uint32_t* const vals_b = (uint32_t*)(bin + B.vals_b);
    RasterParams pg = p;                       // the guarded kernels' view of the parameters
    pg.spec_fail = fail;
    SliceList vl{nullptr, nullptr};
    if (pl.kind == 2) {
      // the kernels declined the slice last time: assume they do again, single pass over the visible list
      if ((rc = cull_stage(f, pl.kind, !immediate, fail, BwdInfoInit{bwd_info, slot_grads, capS, immediate ? 0u : 1u})) != RTGS_OK)
        return rc;
      prof_mark(c, EV_PRE, st);
      // (the decision - is the slice still declined? - is re-derived inside visible_compact: no slice_compact launch)
      const SliceSel sel1 = slice_sel(f);
      vl = SliceList{(const uint32_t*)(f.geom + G.vis_ids), f.slice_ctr + 4};
      launch_visible_compact(P, f.zbin, (uint32_t*)(f.geom + G.vis_ids), f.slice_ctr + 4, f.tiles_touched, f.offsets, f.slice_ctr + 5,
                             fail, st, &sel1, (int32_t*)(f.slice_ctr + 3), fail);
      shade(f, pg, vl, sel1, (size_t)P);
    } else {
      preprocess_all(f, nullptr, true);
      if (!immediate && (rc = scan_slots(f)) != RTGS_OK) return rc;       // gradient-slot bases: only a backward reads them
      prof_mark(c, EV_PRE, st);
    }
    const SliceSel sel2{0, nullptr, nullptr, 0u, 0u, f.slice_ctr, nullptr, f.uv, nullptr, 0u, 0};
    const int32_t* const still_declined = pl.kind == 2 ? (const int32_t*)(f.slice_ctr + 3) : nullptr;
    if (seg2) {
      if (pl.kind != 2)
        hipLaunchKernelGGL(bwd_info_kernel, dim3(1), dim3(1), 0, st, bwd_info, slot_grads, capS, immediate ? 0u : 1u);
      launch_bin_place(pg, f.splats, f.radii, f.tile_mask, f.tile_count, keys_a, seg2, fail, sel2, vl, (size_t)P, st);
      prof_mark(c, EV_SCAN, st); prof_mark(c, EV_BIN0, st); prof_mark(c, EV_EMIT, st);
      const BinFinish fin{f.tile_count, ntiles, f.info, f.info_host, f.slice_ctr + 5, nullptr, f.slice_ctr + 4, c->seq,
                          SpecCaps{fail, 0xffffffffu, capL, immediate ? 0xffffffffu : capS, still_declined}};
      launch_bin_tilesort(ntiles, capL, f.ranges, keys_a, vals_b, fail, st, f.tile_count, seg2, f.ranges, &fin);
    } else {
      uint16_t* const counts = vl.ids ? (uint16_t*)(f.geom + G.block_counts_vis) : f.block_counts;
      if (launch_bin_count(pg, f.splats, f.radii, f.tile_mask, f.tile_count, counts, sel2, vl, (size_t)P, st) != 0)
        return RTGS_E_HIP;
      const SpecCaps caps{fail, capR, capL, immediate ? 0xffffffffu : capS, still_declined};
      launch_bin_tilescan(ntiles, f.tile_count, f.ranges, f.cursor, f.info, f.info_host, nullptr, nullptr,
                          vl.ids ? f.slice_ctr + 5 : f.offsets + (P - 1), vl.ids ? nullptr : f.tiles_touched + (P - 1), c->seq,
                          caps, st);
      prof_mark(c, EV_SCAN, st);
      if (pl.kind != 2) hipLaunchKernelGGL(bwd_info_kernel, dim3(1), dim3(1), 0, st, bwd_info, slot_grads, capS, 1u);
      prof_mark(c, EV_BIN0, st);
      launch_bin_scatter(pg, f.splats, f.radii, f.tile_mask, counts, f.cursor, keys_a, sel2, vl, (size_t)P, st);
      prof_mark(c, EV_EMIT, st);
      launch_bin_tilesort(ntiles, capL, f.ranges, keys_a, vals_b, fail, st);
    }
    prof_mark(c, EV_SORT, st);
    prof_mark(c, EV_BLEND0, st);
    blend(f, pg, f.ranges, vals_b, SlicePass{0, nullptr, nullptr, nullptr, nullptr}, seg2);
    prof_mark(c, EV_BLEND, st);
    c->hint_slice_lists = false; c->hint_main_lists = true;
    c->slice_stats[0] = pl.kind == 2 ? 1 : 0; c->slice_stats[1] = 0; c->slice_stats[2] = 0;
    c->slice_stats[3] = pl.kind == 2 ? (int64_t)ntiles : 0;
  }
  HIP_TRY(hipGetLastError());
  c->hint_geom = f.geom; c->hint_walk = f.fwd_walk;
  if (!immediate) {
    c->spec.pending = true; c->spec.kind = pl.kind; c->spec.seq = c->seq; c->spec.capR = seg_main ? 0xffffffffu : capR; c->spec.capL = capL;
    c->spec.capS = capS; c->spec.geom = f.geom; c->spec.fail_dev = fail; c->spec.stream = (void*)st; c->spec.ntiles = ntiles;
    c->spec.G_total = (int64_t)G.total; c->spec.B_total = (int64_t)B.total; c->spec.I_total = (int64_t)I.total;
    ++c->spec_stats[0];
    *f.num_rendered_host = (int64_t)pl.R + (int64_t)pl.R1;      // the last verified call's; the exact number comes with verify
    if (*f.num_rendered_host < 1) *f.num_rendered_host = 1;
    return RTGS_OK;
  }
  // immediate: the blend is on its way; the totals were published before it started
  if ((rc = wait_published(f)) != RTGS_OK) return rc;
  const uint32_t* pub = f.pub;
  const bool ok = (seg_main || pub[0] <= capR) && pub[1] <= capL && (pl.kind != 2 || (int32_t)pub[6] < 0);
  ++c->plain_stats[0];
  if (!ok) {
    // wrong guess: every guarded kernel after the one that noticed returned at once; start over on the classic path
    pp.valid = false;
    ++c->plain_stats[1];
    outcome = SPEC_REDO;
    return RTGS_OK;
  }
  pp.note(pub[0], pub[1], 0u);
  c->last_listed = pub[2];
  c->plan.valid = false;             // as after every forward without a backward (see the end of forward_classic)
  record_stats(c, (int64_t)pub[0], ntiles, (int64_t)G.total, (int64_t)B.total, (int64_t)I.total, true, (int64_t)pub[1]);
  *f.num_rendered_host = (int64_t)pub[0];
  return RTGS_OK;
}

// The classic forward: the host waits for the totals it sizes the next stage by (the slice's decision when it asks first,
// the tiles the slice left, {R, longest list, gradient slots} of the main pass), falls back to the global radix sort when a
// tile list is too long for the LDS sort, and leaves the statistics, the hints for the backward and the plans behind.
static int forward_classic(FwdCall& f, bool sort_path, bool sliced) {
  rtgs_ctx* const c = f.c; const rtgs_raster_settings* const s = f.s;
  const RasterParams& p = f.p; const GeomLayout& G = f.G;
  const int32_t P = p.P; const int ntiles = f.ntiles; const bool want_bwd = f.want_bwd; hipStream_t st = f.st;
  int rc;
  const bool sliced0 = sliced;                 // what this call started as (the variable follows the passes below)
  int64_t R = 0, R1 = 0;
  uint32_t longest = 0, slots = 0, n_left = 0, n_fin = 0, slice_longest = 0;
  SlicePass pass{0, nullptr, nullptr, nullptr, nullptr};
  bool declined = false, considered = false;
  SliceList vis{nullptr, nullptr};             // every visible Gaussian, when the declined single pass built the list
  const int32_t* mask_main = f.tile_mask;      // tile mask of the pass that ends in the host sync
  if (P == 0) HIP_TRY(hipMemsetAsync(f.zero_words, 0, (size_t)f.zero_n * sizeof(uint32_t), st));   // ranges1_bwd for the backward
  if (P > 0) {
    if (sort_path) {   // only the fallback path needs the 3-sigma-rect tile counts
      launch_mask_sat(f.tile_mask, p.gx, p.gy, f.sat, st);
      DBG(s, st);
    }
    const SliceSel sel1 = slice_sel(f);
    if (!sliced) {
      preprocess_all(f, sort_path ? f.sat : nullptr, true);
      if (!sort_path && want_bwd && (rc = scan_slots(f)) != RTGS_OK) return rc;
    } else {
      // geometry of every Gaussian now, Splat records only where a list will read them
      launch_preprocess_cull(p, f.means3D, f.scales, f.rotations, f.tiles_touched, f.radii, f.out_radii, f.zero_words, f.zero_n,
                             f.zbin, f.uv, f.slice_hist, st);
    }
    DBG(s, st);
    prof_mark(c, EV_PRE, st);
    if (sliced) {
      launch_slice_hist(P, f.zbin, f.tiles_touched, f.radii, f.slice_hist, f.slice_cover, st);
      const bool ask = f.slice_auto && c->ask_first;
      if (ask) next_seq(c);
      launch_slice_compact(P, sel1, (uint32_t*)(f.geom + G.slice_ids), f.slice_ctr + 2, f.tiles_touched, f.offsets,
                           f.slice_ctr + 4, ask ? f.info_host : nullptr, c->seq, nullptr, st);
      if (ask) {
        if ((rc = wait_published(f)) != RTGS_OK) return rc;
        declined = (int32_t)f.pub[6] < 0;
      }
    }
    if (sliced && declined) {
      // the kernels declined the slice and the host knows: shade every visible Gaussian and go on as a single pass
      // ... through a compact list of the visible ones (dense lanes in the shade / count / scatter kernels)
      vis = SliceList{(const uint32_t*)(f.geom + G.vis_ids), f.slice_ctr + 4};
      launch_visible_compact(P, f.zbin, (uint32_t*)(f.geom + G.vis_ids), f.slice_ctr + 4, f.tiles_touched, f.offsets,
                             f.slice_ctr + 5, nullptr, st);
      shade(f, p, vis, sel1, (size_t)P);
      sliced = false;
      considered = true;
    }
    if (sliced) {
      // Pass 1.  Tiles whose every pixel saturates inside the slice are final; blend_fwd leaves a tile mask of the others.
      next_seq(c);
      if ((rc = slice_pass1(f, nullptr)) != RTGS_OK) return rc;
      // the forward's host sync: the last tile of the slice publishes how many tiles are left
      if ((rc = wait_published(f)) != RTGS_OK) return rc;
      n_left = f.pub[2]; n_fin = f.pub[3];
      R1 = (int64_t)f.pub[4];          // total of the slice lists, finished or not (accounting only)
      slice_longest = f.pub[1];        // (per-tile segments; 0 otherwise)
      if (n_left > 0) {
        mask_main = f.mask2;
        pass = SlicePass{2, nullptr, f.mask2, nullptr, nullptr};
        // pass 2 bins against the whole map, but only Gaussians whose tile rect holds an unfinished tile (summed-area
        // table of the pass-2 mask) are shaded and enumerated
        launch_mask_sat(f.mask2, p.gx, p.gy, f.sat, st);
        SliceSel sel_rest = sel1;
        sel_rest.sat = f.sat; sel_rest.uv = f.uv;
        shade(f, p, SliceList{nullptr, nullptr}, sel_rest, 0);
        if (want_bwd && (rc = scan_slots(f)) != RTGS_OK) return rc;
      } else if (want_bwd) {
        // every tile is final: only the slice's Gaussians can receive gradient; slice_compact already laid their slot
        // runs out (gbase in `offsets`), and the sum of their rect areas is within the slice's instance budget by
        // construction of the cut - no scan over the map, no host round trip for the size
        slots = (uint32_t)G.slice_cap;
      }
    }
    if (!sort_path && !(sliced && n_left == 0)) {
      // exact per-tile counts -> ranges; the one host sync of the forward sizes the instance arrays
      const SliceSel sel2{sliced ? 2 : 0, nullptr, nullptr, 0u, 0u, f.slice_ctr, sliced ? f.sat : nullptr, f.uv, nullptr, 0u, 0};
      if (launch_bin_count(p, f.splats, f.radii, mask_main, f.tile_count,
                           vis.ids ? (uint16_t*)(f.geom + G.block_counts_vis) : f.block_counts, sel2, vis, (size_t)P, st) != 0)
        return RTGS_E_HIP;
      next_seq(c);
      launch_bin_tilescan(ntiles, f.tile_count, f.ranges, f.cursor, f.info, f.info_host, nullptr, nullptr,
                          // size of the gradient-slot space: the cursor visible_compact advanced, or the end of the full scan
                          want_bwd ? (vis.ids ? f.slice_ctr + 5 : f.offsets + (P - 1)) : nullptr,
                          want_bwd && !vis.ids ? f.tiles_touched + (P - 1) : nullptr, c->seq,
                          SpecCaps{nullptr, 0u, 0u, 0u, nullptr}, st);
      DBG(s, st);
      prof_mark(c, EV_SCAN, st);
      if ((rc = wait_published(f)) != RTGS_OK) return rc;
      R = (int64_t)f.pub[0];
      longest = f.pub[1];
      slots = f.pub[5];
      if ((int)longest > bin_sort_capacity()) {   // a tile list too long for the LDS sort: redo with rect counts
        sort_path = true;
        if (sliced) {         // the global-sort path renders every tile itself: drop the slice's results
          HIP_TRY(hipMemsetAsync(f.ranges1_bwd, 0, (size_t)ntiles * sizeof(uint2), st));
          sliced = false; R1 = 0; n_left = n_fin = 0;
          pass = SlicePass{0, nullptr, nullptr, nullptr, nullptr};
          mask_main = f.tile_mask;
        }
        launch_mask_sat(f.tile_mask, p.gx, p.gy, f.sat, st);
        preprocess_all(f, f.sat, false);
        DBG(s, st);
      }
    }
    if (sort_path) {
      size_t tb = G.scan_temp_bytes;
      HIP_TRY(rocprim::inclusive_scan(f.geom + G.scan_temp, tb, f.tiles_touched, f.offsets, (size_t)P, rocprim::plus<uint32_t>(), st));
      uint32_t total = 0;
      HIP_TRY(hipMemcpyAsync(&total, f.offsets + (P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      prof_mark(c, EV_SCAN, st);
      HIP_TRY(hipStreamSynchronize(st));
      R = (int64_t)total;
    }
  }
  *f.num_rendered_host = R + R1;

  const bool use_slots = want_bwd && !sort_path && slots > 0 && slots <= SLOTS_MAX;
  const BinLayout B = bin_layout(R, ntiles, sort_path, use_slots ? (size_t)slots : 0);
  char* bin = (char*)f.binning_resize(f.binning_user, B.total);
  if (!bin) return RTGS_E_ALLOC;
  c->last_bin = bin;
  hipLaunchKernelGGL(bwd_info_kernel, dim3(1), dim3(1), 0, st, (BwdInfo*)(f.img + f.I.bwd_info),
                     (SplatGrad*)(bin + B.slot_grads), use_slots ? slots : 0u, use_slots ? 1u : 0u);
  uint64_t *keys_a = (uint64_t*)(bin + B.keys_a), *keys_b = (uint64_t*)(bin + B.keys_b);
  uint32_t *vals_a = (uint32_t*)(bin + B.vals_a), *vals_b = (uint32_t*)(bin + B.vals_b);
  if (P == 0 || sort_path) HIP_TRY(hipMemsetAsync(f.ranges, 0, (size_t)ntiles * sizeof(uint2), st));
  if (R > 0 && !sort_path) {
    prof_mark(c, EV_BIN0, st);
    launch_bin_scatter(p, f.splats, f.radii, mask_main, vis.ids ? (const uint16_t*)(f.geom + G.block_counts_vis) : f.block_counts,
                       f.cursor, (unsigned long long*)keys_a,
                       SliceSel{sliced ? 2 : 0, nullptr, nullptr, 0u, 0u, f.slice_ctr, sliced ? f.sat : nullptr, f.uv, nullptr, 0u, 0},
                       vis, (size_t)P, st);
    DBG(s, st);
    prof_mark(c, EV_EMIT, st);
    launch_bin_tilesort(ntiles, longest, f.ranges, (const unsigned long long*)keys_a, vals_b, nullptr, st);
    DBG(s, st);
    prof_mark(c, EV_SORT, st);
  } else if (R > 0) {
    prof_mark(c, EV_BIN0, st);
    launch_emit_keys(p, f.splats, f.radii, f.offsets, f.tile_mask, keys_a, vals_a, st);
    DBG(s, st);
    prof_mark(c, EV_EMIT, st);
    size_t tb = B.sort_temp_bytes;
    HIP_TRY(rocprim::radix_sort_pairs(bin + B.sort_temp, tb, keys_a, keys_b, vals_a, vals_b, (size_t)R, 0u,
                                      (unsigned)(32 + bits_for((uint32_t)ntiles)), st));
    DBG(s, st);
    prof_mark(c, EV_SORT, st);
    launch_tile_ranges(R, keys_b, f.ranges, st);
    DBG(s, st);
    prof_mark(c, EV_RANGES, st);
  }
  prof_mark(c, EV_BLEND0, st);
  if (!sliced || n_left > 0)     // pass 2 (or the only pass); with every tile finished by the slice there is nothing to draw
    blend(f, p, f.ranges, vals_b, pass, 0u);
  prof_mark(c, EV_BLEND, st);
  DBG(s, st);
  HIP_TRY(hipGetLastError());
  record_stats(c, R + R1, ntiles, (int64_t)G.total, (int64_t)B.total, (int64_t)f.I.total, !sort_path, (int64_t)longest);
  c->slice_stats[0] = (sliced || considered) ? 1 : 0; c->slice_stats[1] = R1; c->slice_stats[2] = n_fin;
  c->slice_stats[3] = considered ? (int64_t)ntiles : (int64_t)n_left;      // declined: every tile goes to the single pass
  if (f.slice_auto && (sliced || considered)) c->ask_first = considered || (R1 == 0 && n_fin == 0);
  // which of the two list sets the backward of THIS forward has to walk (host-side hint, keyed by the geometry buffer)
  c->hint_geom = f.geom; c->hint_slice_lists = sliced && n_fin > 0; c->hint_main_lists = R > 0; c->hint_walk = f.fwd_walk;
  // What a speculative forward on this context may assume next time (rtgs_raster_forward_verify keeps it current).  From the
  // FINAL state of this call: a forward that fell back to the global sort (a list longer than the LDS sort holds) leaves no
  // plan - speculating on it would fail its guard word on every step and run every step twice
  note_plan(c->plan, f, c->plan.P == P, sort_path ? -1 : ((sliced && n_left == 0) ? 1 : (considered ? 2 : (!sliced && P > 0 ? 0 : -1))),
            want_bwd, R, longest, slots);
  c->plan.R1 = (uint32_t)R1; c->plan.n_fin = n_fin;
  c->plan.note_slice(slice_longest);      // (after a failed tile gather: the list that outgrew the blend's arena)
  // ... and what the next forward WITHOUT a backward on this image may assume (any Gaussian count)
  if (!want_bwd)
    note_plan(sliced0 ? c->plan_plain : c->plan_plain0, f, true, sort_path ? -1 : (sliced0 ? (considered ? 2 : -1) : (P > 0 ? 0 : -1)),
              true, R, longest, 0u);
  return RTGS_OK;
}

}  // namespace rtgs

using namespace rtgs;

extern "C" {

const char* rtgs_version(void) { return "rtgs-hip 0.2.0 (gfx950)"; }

rtgs_ctx* rtgs_ctx_create(void) {
  rtgs_ctx* c = new (std::nothrow) rtgs_ctx();
  if (c) c->sw = default_ctx()->sw;
  return c;
}
void rtgs_ctx_destroy(rtgs_ctx* c) {
  if (!c || c == default_ctx()) return;
  if (c->ev_init) for (int i = 0; i < EV_N; ++i) (void)hipEventDestroy(c->ev[i]);
  if (c->info_host) (void)hipHostFree(c->info_host);
  if (c->cull.scratch) (void)hipFree(c->cull.scratch);
  if (c->cull.mismatches) (void)hipFree(c->cull.mismatches);
  if (c->fsort_cls) (void)hipFree(c->fsort_cls);
  delete c;
}

size_t rtgs_raster_geom_bytes_ctx(rtgs_ctx* c, int32_t P, int32_t H, int32_t W) {
  return geom_layout(P, (W + TILE - 1) / TILE, (H + TILE - 1) / TILE, use(c)->sw.slice_budget).total;
}
size_t rtgs_raster_geom_bytes(int32_t P, int32_t H, int32_t W) { return rtgs_raster_geom_bytes_ctx(nullptr, P, H, W); }
size_t rtgs_raster_binning_bytes(int64_t R, int32_t H, int32_t W) {
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  return bin_layout(R, gx * gy, true, 0).total;
}
size_t rtgs_raster_image_bytes(int32_t H, int32_t W) {
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  return img_layout(H, W, gx * gy).total;
}
// [P x SplatGrad (64 B)] [P x touched byte]
size_t rtgs_raster_backward_scratch_bytes(int32_t P) {
  const size_t n = (size_t)(P > 0 ? P : 1);
  return align_up(n * sizeof(SplatGrad)) + align_up(n);
}

int rtgs_raster_last_stats_ctx(rtgs_ctx* c, int64_t* out) {
  if (!out) return RTGS_E_INVALID;
  memcpy(out, use(c)->stats, sizeof(use(c)->stats));
  return RTGS_OK;
}
void rtgs_raster_set_counters_ctx(rtgs_ctx* c, void* counters) { use(c)->counters = (unsigned long long*)counters; }

int rtgs_raster_forward_ctx(rtgs_ctx* ctx, const rtgs_raster_settings* s, int32_t P, int32_t M, const float* means3D,
                            const float* opacities, const float* shs, const float* scales, const float* rotations,
                            const float* normal_w, const int32_t* tile_mask, float* out_color, float* out_depth,
                            int32_t* out_cidx, int32_t* out_didx, float* out_cw, float* out_dw, float* out_T,
                            int32_t* out_radii, rtgs_resize_fn geom_resize, void* geom_user,
                            rtgs_resize_fn binning_resize, void* binning_user, rtgs_resize_fn image_resize,
                            void* image_user, int64_t* num_rendered_host, int32_t flags, void* stream) {
  rtgs_ctx* c = use(ctx);
  FwdCall f;
  f.c = c;
  // 1. The context's one-shot state is consumed HERE, before any early return - a refused forward must not leave the
  // pointer armed for the next, unrelated forward on this context.  The cull cache: every forward disarms it;
  // only the speculative kinds 1 and 2 arm it again (or find it armed).
  f.aux_zero = c->aux_zero; c->aux_zero = nullptr;
  f.cull_epoch = c->cull.next_epoch; c->cull.next_epoch = 0;
  f.cull_was_armed = c->cull.armed; c->cull.armed = false;
  if (f.cull_was_armed) ++c->cull.stats[2];
  // 2. validate
  int rc = make_params(s, P, M, f.p);
  if (rc != RTGS_OK) return rc;
  if (P > 0 && (!means3D || !opacities || !shs || !scales || !rotations || !normal_w)) return RTGS_E_INVALID;
  if (!tile_mask || !out_color || !out_depth || !out_cidx || !out_didx || !out_cw || !out_dw || !out_T)
    return RTGS_E_INVALID;
  if (!geom_resize || !binning_resize || !image_resize || !num_rendered_host) return RTGS_E_INVALID;
  // 3. set up the call: the caller's arguments, then the buffers (geometry and image callbacks) and what is derived
  f.s = s; f.st = (hipStream_t)stream; f.flags = flags; f.want_bwd = !(flags & RTGS_FWD_NO_BACKWARD);
  f.means3D = means3D; f.opacities = opacities; f.shs = shs; f.scales = scales; f.rotations = rotations; f.normal_w = normal_w;
  f.tile_mask = tile_mask;
  f.out_color = out_color; f.out_depth = out_depth; f.out_cidx = out_cidx; f.out_didx = out_didx; f.out_cw = out_cw;
  f.out_dw = out_dw; f.out_T = out_T; f.out_radii = out_radii;
  f.geom_resize = geom_resize; f.geom_user = geom_user; f.binning_resize = binning_resize; f.binning_user = binning_user;
  f.image_resize = image_resize; f.image_user = image_user; f.num_rendered_host = num_rendered_host;
  if ((rc = forward_setup(f)) != RTGS_OK) return rc;
  if (c->spec.pending) return RTGS_E_INVALID;          // the previous speculative forward was never verified
  c->spec.geom = nullptr; c->spec.fail_dev = nullptr;
  const bool sort_path = (size_t)f.ntiles > bin_lds_limit_tiles() || c->force_sort_path;
  // near-slice pass: mode 1 forces it (tests); automatic mode considers it on large maps only, and there the kernels
  // decide from the depth histograms whether it runs (an empty slice sends every tile to the second pass)
  const bool sliced = !sort_path && P > 0 && (c->sw.slice_mode == 1 || (f.slice_auto && P >= large_map_min() && f.ntiles >= 256));
  // 4. the speculative / immediate path, if this call may take it ...
  SpecOutcome outcome;
  rc = forward_speculative(f, sort_path, sliced, outcome);
  if (outcome == SPEC_RETURNED) return rc;
  // 5. ... else (or after an immediate guess that did not hold) the classic path, which ends with 6. the bookkeeping
  return forward_classic(f, sort_path, sliced);
}

static int backward_impl(rtgs_ctx* ctx, const rtgs_raster_settings* s, int32_t P, int32_t M, int64_t R, const float* means3D,
                         const float* opacities, const float* shs, const float* scales, const float* rotations,
                         const float* normal_w, void* geom_buffer, void* binning_buffer,
                         const void* image_buffer, const float* out_color, const float* out_T,
                         const int32_t* out_didx,
                         const float* dL_dcolor, const float* dL_ddepth, float* dL_dmeans3D, float* dL_dopacities,
                         float* dL_dshs, float* dL_dscales, float* dL_drotations, float* dL_dnormal_w,
                         void* grad_scratch, uint8_t* row_state, int32_t train_begin, int32_t train_end, void* stream,
                         bool walk_only = false, const rtgs_loss_signs* lsg = nullptr) {
  rtgs_ctx* c = use(ctx);   // NOTE: the geometry buffer is written here (slot counters): it is scratch of the pair
  RasterParams p;
  int rc = make_params(s, P, M, p);
  if (rc != RTGS_OK) return rc;
  if (P == 0) return RTGS_OK;
  // the backward of a speculative forward guards itself with that forward's device word (see rtgs_raster_forward_verify)
  if (c->spec.geom == geom_buffer && c->spec.fail_dev) p.spec_fail = c->spec.fail_dev;
  if (!means3D || !opacities || !shs || !scales || !rotations || !normal_w || !geom_buffer || !binning_buffer ||
      !image_buffer || !out_color || !out_T || !out_didx || (!lsg && (!dL_dcolor || !dL_ddepth)) || !grad_scratch || R < 0)
    return RTGS_E_INVALID;
  // signs in place of the gradient images: only the entry walk reads them, so the forward must be remembered as all-entry
  if (lsg && (!walk_only || !lsg->signs || !lsg->sums || c->hint_geom != geom_buffer || c->hint_walk != 2)) return RTGS_E_INVALID;
  const LossSigns lsd = lsg ? LossSigns{lsg->signs, lsg->sums, lsg->color_weight, lsg->depth_weight, lsg->loss_out4}
                            : LossSigns{nullptr, nullptr, 0.f, 0.f, nullptr};
  int entry_launches = 0;
  if (!walk_only && (!dL_dmeans3D || !dL_dopacities || !dL_dshs || !dL_dscales || !dL_drotations || !dL_dnormal_w)) return RTGS_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int ntiles = p.gx * p.gy;
  const GeomLayout G = geom_layout(P, p.gx, p.gy, 1);   // only budget-independent offsets are read here
  const BinLayout B = bin_layout(R, ntiles, false, 0);  // point_list sits at offset 0 in every layout
  const ImgLayout I = img_layout(p.H, p.W, ntiles);
  const char* geom = (const char*)geom_buffer;
  const char* bin = (const char*)binning_buffer;
  const char* img = (const char*)image_buffer;
  SplatGrad* grads = (SplatGrad*)grad_scratch;
  for (int i = EV_B0; i < EV_N; ++i) c->ev_set[i] = false;
  prof_mark(c, EV_B0, st);
  uint8_t* touched = (uint8_t*)grad_scratch + align_up((size_t)P * sizeof(SplatGrad));
  // row-state mode: the caller zeroed the scratch once and preprocess_bwd re-zeroes every line it consumes
  if (!row_state) HIP_TRY(hipMemsetAsync(grads, 0, rtgs_raster_backward_scratch_bytes(P), st));
  const BwdInfo* binfo = (const BwdInfo*)(img + I.bwd_info);
  const uint32_t* gbase = (const uint32_t*)(geom + G.offsets);
  const int32_t* radii = (const int32_t*)(geom + G.radii);
  uint32_t* slot_count = (uint32_t*)(geom + G.slot_count);      // scratch of the backward inside the geometry buffer
  const uint32_t* tile_mode = (const uint32_t*)(img + I.tile_mode);   // per tile: which of the two walks (blend_fwd decided)
  if (R > 0) {
    // two-pass forward: tiles the near slice finished walk its lists (ranges1_bwd is all-empty otherwise, and a
    // workgroup with an empty range returns at once); every other tile walks the main lists
    // (a launch whose every workgroup would find an empty range is skipped when this context still remembers the forward)
    const bool hinted = c->hint_geom == geom_buffer;
    // bit 0 strip, bit 1 row-granular, bit 2 MFMA walk: a forced walk launches only its kernel
    // the kernels to launch follow what the FORWARD wrote into tile_mode (remembered with its geometry buffer), not the
    // context's setting at backward time; a backward this context does not remember launches all three - each kernel
    // takes only the tiles that carry its walk
    const int which = !hinted ? 7 : (c->hint_walk == 2 ? 4 : (c->hint_walk == -1 ? 3 : (c->hint_walk == 0 ? 1 : 2)));
    if (train_begin < 0 || train_end > P || train_end < train_begin) return RTGS_E_INVALID;
    const uint32_t t0 = (uint32_t)train_begin, tn = (uint32_t)(train_end - train_begin);   // trainable rows (the rest: rendered only)
    const uint32_t* depth_pos = (const uint32_t*)(img + I.depth_pos);
    for (int set = 0; set < 2; ++set) {
      if (hinted && !(set == 0 ? c->hint_slice_lists : c->hint_main_lists)) continue;
      const uint2* rg = set == 0 ? (const uint2*)(geom + G.ranges1_bwd) : (const uint2*)(img + I.ranges);
      const uint32_t* pl = set == 0 ? (const uint32_t*)(geom + G.list1) : (const uint32_t*)(bin + B.vals_b);
      if (which & 3)
        launch_blend_bwd(p, rg, pl, (const Splat*)(geom + G.splats), out_color, out_T, (const uint32_t*)(img + I.n_contrib),
                         out_didx, dL_dcolor, dL_ddepth, gbase, slot_count, binfo, grads, touched, tile_mode, which & 3, t0, tn, st);
      if (which & 4) ++entry_launches;
      if (which & 4)
        launch_blend_bwd_entry(p, rg, pl, (const Splat*)(geom + G.splats), out_color, (const uint32_t*)(img + I.n_contrib),
                               out_didx, depth_pos, (const uint32_t*)(img + I.tile_last), dL_dcolor, dL_ddepth, gbase, slot_count, binfo, grads,
                               touched, tile_mode, t0, tn,
                               TileCache{(float4*)(img + I.tile_recs), (uint16_t*)(img + I.tile_masks), (float2*)(img + I.depth_aux)},
                               set == 0 ? (uint32_t)(BLOCK / 4) : (uint32_t)BLOCK,      // the near slice's first batch is a quarter batch
                               st, lsg ? &lsd : nullptr);
    }
    prof_mark(c, EV_BWALK, st);
    // sum each touched Gaussian's slots into its SplatGrad record (no-op on the atomic fallback)
    if (!walk_only) launch_grad_reduce(P, touched, gbase, slot_count, binfo, grads, p.spec_fail, st);
    DBG(s, st);
  }
  prof_mark(c, EV_BBLEND, st);
  if (lsg && lsg->loss_out4 && entry_launches == 0) {     // nothing to walk: nobody has written the loss values yet
    const rtgs_loss_cfg lc{lsg->color_weight, lsg->depth_weight, 0.f, 0.f, nullptr, 0};
    if (rtgs_slam_loss_values(&lc, lsg->sums, lsg->loss_out4, stream) != 0) return RTGS_E_HIP;
  }
  if (walk_only) { prof_mark(c, EV_BPRE, st); HIP_TRY(hipGetLastError()); return RTGS_OK; }   // a fused consumer takes over
  launch_preprocess_bwd(p, means3D, opacities, shs, scales, rotations, normal_w, radii,
                        (const uint8_t*)(geom + G.clamped), grads, touched, row_state, dL_dmeans3D, dL_dopacities,
                        dL_dshs, dL_dscales, dL_drotations, dL_dnormal_w, st);
  prof_mark(c, EV_BPRE, st);
  DBG(s, st);
  HIP_TRY(hipGetLastError());
  return RTGS_OK;
}

int rtgs_raster_backward_ctx(rtgs_ctx* ctx, const rtgs_raster_settings* s, int32_t P, int32_t M, int64_t R,
                             const float* means3D, const float* opacities, const float* shs, const float* scales,
                             const float* rotations, const float* normal_w, void* geom_buffer,
                             void* binning_buffer, const void* image_buffer, const float* out_color,
                             const float* out_T, const int32_t* out_didx, const float* dL_dcolor, const float* dL_ddepth,
                             float* dL_dmeans3D, float* dL_dopacities, float* dL_dshs, float* dL_dscales,
                             float* dL_drotations, float* dL_dnormal_w, void* grad_scratch, void* stream) {
  return backward_impl(ctx, s, P, M, R, means3D, opacities, shs, scales, rotations, normal_w, geom_buffer, binning_buffer,
                       image_buffer, out_color, out_T, out_didx, dL_dcolor, dL_ddepth, dL_dmeans3D, dL_dopacities,
                       dL_dshs, dL_dscales, dL_drotations, dL_dnormal_w, grad_scratch, nullptr, 0, P, stream);
}

int rtgs_raster_backward_rows_ctx(rtgs_ctx* ctx, const rtgs_raster_settings* s, int32_t P, int32_t M, int64_t R,
                                  const float* means3D, const float* opacities, const float* shs, const float* scales,
                                  const float* rotations, const float* normal_w, void* geom_buffer,
                                  void* binning_buffer, const void* image_buffer, const float* out_color,
                                  const float* out_T, const int32_t* out_didx, const float* dL_dcolor,
                                  const float* dL_ddepth, float* dL_dmeans3D, float* dL_dopacities, float* dL_dshs,
                                  float* dL_dscales, float* dL_drotations, float* dL_dnormal_w, void* grad_scratch,
                                  uint8_t* row_state, void* stream) {
  return rtgs_raster_backward_range_ctx(ctx, s, P, M, R, means3D, opacities, shs, scales, rotations, normal_w, geom_buffer,
                                        binning_buffer, image_buffer, out_color, out_T, out_didx, dL_dcolor, dL_ddepth,
                                        dL_dmeans3D, dL_dopacities, dL_dshs, dL_dscales, dL_drotations, dL_dnormal_w,
                                        grad_scratch, row_state, 0, P, stream);
}

int rtgs_raster_backward_range_ctx(rtgs_ctx* ctx, const rtgs_raster_settings* s, int32_t P, int32_t M, int64_t R,
                                   const float* means3D, const float* opacities, const float* shs, const float* scales,
                                   const float* rotations, const float* normal_w, void* geom_buffer,
                                   void* binning_buffer, const void* image_buffer, const float* out_color,
                                   const float* out_T, const int32_t* out_didx, const float* dL_dcolor,
                                   const float* dL_ddepth, float* dL_dmeans3D, float* dL_dopacities, float* dL_dshs,
                                   float* dL_dscales, float* dL_drotations, float* dL_dnormal_w, void* grad_scratch,
                                   uint8_t* row_state, int32_t train_begin, int32_t train_end, void* stream) {
  if (P > 0 && !row_state) return RTGS_E_INVALID;
  return backward_impl(ctx, s, P, M, R, means3D, opacities, shs, scales, rotations, normal_w, geom_buffer, binning_buffer,
                       image_buffer, out_color, out_T, out_didx, dL_dcolor, dL_ddepth, dL_dmeans3D, dL_dopacities,
                       dL_dshs, dL_dscales, dL_drotations, dL_dnormal_w, grad_scratch, row_state, train_begin, train_end, stream);
}

int rtgs_raster_backward_walk_ctx(rtgs_ctx* ctx, const rtgs_raster_settings* s, int32_t P, int32_t M, int64_t R,
                                   const float* means3D, const float* opacities, const float* shs, const float* scales,
                                   const float* rotations, const float* normal_w, void* geom_buffer,
                                   void* binning_buffer, const void* image_buffer, const float* out_color,
                                   const float* out_T, const int32_t* out_didx, const float* dL_dcolor,
                                   const float* dL_ddepth, float* dL_dmeans3D, float* dL_dopacities, float* dL_dshs,
                                   float* dL_dscales, float* dL_drotations, float* dL_dnormal_w, void* grad_scratch,
                                   uint8_t* row_state, int32_t train_begin, int32_t train_end, void* stream) {
  return backward_impl(ctx, s, P, M, R, means3D, opacities, shs, scales, rotations, normal_w, geom_buffer, binning_buffer,
                       image_buffer, out_color, out_T, out_didx, dL_dcolor, dL_ddepth, dL_dmeans3D, dL_dopacities,
                       dL_dshs, dL_dscales, dL_drotations, dL_dnormal_w, grad_scratch, row_state, train_begin, train_end, stream, true);
}

int rtgs_raster_backward_walk_signs_ctx(rtgs_ctx* ctx, const rtgs_raster_settings* s, int32_t P, int32_t M, int64_t R,
                                        const float* means3D, const float* opacities, const float* shs, const float* scales,
                                        const float* rotations, const float* normal_w, void* geom_buffer, void* binning_buffer,
                                        const void* image_buffer, const float* out_color, const float* out_T,
                                        const int32_t* out_didx, const rtgs_loss_signs* loss, void* grad_scratch,
                                        uint8_t* row_state, int32_t train_begin, int32_t train_end, void* stream) {
  if (!loss || (P > 0 && !row_state)) return RTGS_E_INVALID;
  return backward_impl(ctx, s, P, M, R, means3D, opacities, shs, scales, rotations, normal_w, geom_buffer, binning_buffer,
                       image_buffer, out_color, out_T, out_didx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr, grad_scratch, row_state, train_begin, train_end, stream, true, loss);
}
int rtgs_raster_signs_ok_ctx(rtgs_ctx* ctx, const void* geom_buffer) {
  rtgs_ctx* c = use(ctx);
  return c->sw.loss_signs && geom_buffer && c->hint_geom == geom_buffer && c->hint_walk == 2 ? 1 : 0;
}
void rtgs_raster_set_loss_signs_ctx(rtgs_ctx* ctx, int enable) { use(ctx)->sw.loss_signs = enable != 0; }
int rtgs_raster_loss_signs_stats_ctx(rtgs_ctx* ctx, int64_t* out2) {
  if (!out2) return RTGS_E_INVALID;
  memcpy(out2, use(ctx)->loss_path_stats, sizeof(use(ctx)->loss_path_stats));
  return RTGS_OK;
}
void rtgs_raster_note_loss_path_ctx(rtgs_ctx* ctx, int signs) { ++use(ctx)->loss_path_stats[signs ? 0 : 1]; }

void rtgs_raster_set_profiling_ctx(rtgs_ctx* c, int enable) { use(c)->prof = enable != 0; }
void rtgs_raster_set_near_slice_ctx(rtgs_ctx* c, int mode, int budget_per_tile) {
  use(c)->sw.slice_mode = mode;
  if (budget_per_tile > 0) use(c)->sw.slice_budget = budget_per_tile;
}
int rtgs_raster_last_slice_stats_ctx(rtgs_ctx* c, int64_t* out) {
  if (!out) return RTGS_E_INVALID;
  memcpy(out, use(c)->slice_stats, sizeof(use(c)->slice_stats));
  return RTGS_OK;
}
void rtgs_raster_force_sort_path_ctx(rtgs_ctx* c, int enable) { use(c)->force_sort_path = enable != 0; }
int rtgs_raster_forward_verify_ctx(rtgs_ctx* ctx, int64_t* num_rendered_host) {
  rtgs_ctx* c = use(ctx);
  if (!c->spec.pending) return 0;
  c->spec.pending = false;
  uint32_t pub[7] = {0, 0, 0, 0, 0, 0, 0};
  const int rc = wait_published_words(c->info_host, c->spec.seq, (hipStream_t)c->spec.stream, pub);
  if (rc != RTGS_OK) { c->plan.valid = false; return rc; }
  rtgs_ctx::Plan& pl = c->plan;
  bool ok;
  if (c->spec.kind == 1) {
    const uint32_t n_left = pub[2];
    ok = n_left == 0u && pub[5] == 0u;           // ... and recull_rows did not see the view move under the cached cull
    if (pub[5] != 0u) ++c->cull.stats[3];
    pl.R1 = pub[4]; pl.n_fin = pub[3]; pl.R = 0; pl.longest = 0;
    pl.note_slice(pub[1]);
    if (c->spec.gathered && pub[1] > (uint32_t)FSORT_CAP) c->gather_blocked = true;
    c->last_listed = pub[0];
    c->slice_stats[1] = pub[4]; c->slice_stats[2] = pub[3]; c->slice_stats[3] = n_left;
  } else {
    ok = pub[0] <= c->spec.capR && pub[1] <= c->spec.capL && pub[5] <= c->spec.capS && (c->spec.kind != 2 || (int32_t)pub[6] < 0) &&
         pub[4] == 0u;
    if (pub[4] != 0u) ++c->cull.stats[3];
    pl.note(pub[0], pub[1], pub[5]); pl.R1 = 0;
    c->last_listed = pub[2];
  }
  record_stats(c, (int64_t)pl.R + (int64_t)pl.R1, c->spec.ntiles, c->spec.G_total, c->spec.B_total, c->spec.I_total, true,
               (int64_t)pl.longest);
  if (num_rendered_host) *num_rendered_host = c->stats[0] > 0 ? c->stats[0] : 1;
  if (!ok) { pl.valid = false; ++c->spec_stats[1]; }
  return ok ? 0 : 1;
}
const uint32_t* rtgs_raster_spec_fail_ptr_ctx(rtgs_ctx* ctx) {
  rtgs_ctx* c = use(ctx);
  return c->spec.pending ? c->spec.fail_dev : nullptr;
}
void rtgs_raster_set_speculation_ctx(rtgs_ctx* ctx, int enable) {
  rtgs_ctx* c = use(ctx);
  c->sw.speculation = enable != 0;
  c->plan = rtgs_ctx::Plan();          // forget the history: the next forward runs plainly and starts it over
}
int rtgs_raster_speculation_stats_ctx(rtgs_ctx* ctx, int64_t* out3) {
  if (!out3) return RTGS_E_INVALID;
  memcpy(out3, use(ctx)->spec_stats, sizeof(use(ctx)->spec_stats));
  return RTGS_OK;
}
int rtgs_raster_plain_stats_ctx(rtgs_ctx* ctx, int64_t* out2) {
  if (!out2) return RTGS_E_INVALID;
  memcpy(out2, use(ctx)->plain_stats, sizeof(use(ctx)->plain_stats));
  return RTGS_OK;
}
void rtgs_raster_set_plain_onepass_ctx(rtgs_ctx* ctx, int enable) {
  rtgs_ctx* c = use(ctx);
  c->sw.plain_onepass = enable != 0;
  c->plan_plain = rtgs_ctx::Plan();
  c->plan_plain0 = rtgs_ctx::Plan();
}
uint32_t rtgs_raster_last_listed_ctx(rtgs_ctx* c) { return use(c)->last_listed; }
void rtgs_raster_set_cull_cache_ctx(rtgs_ctx* ctx, int enable) {
  rtgs_ctx* c = use(ctx);
  c->sw.cull_cache = enable != 0;
  c->cull.armed = false;
}
void rtgs_raster_set_cull_cache_check_ctx(rtgs_ctx* ctx, int enable) { use(ctx)->sw.cull_check = enable != 0; }
void rtgs_raster_set_map_epoch_ctx(rtgs_ctx* ctx, uint64_t epoch) { use(ctx)->cull.next_epoch = epoch; }
uint8_t* rtgs_raster_cull_marks_ctx(rtgs_ctx* ctx) {
  rtgs_ctx* c = use(ctx);
  return c->cull.armed ? c->cull.marks : nullptr;
}
int rtgs_raster_cull_cache_stats_ctx(rtgs_ctx* ctx, int64_t* out5) {
  rtgs_ctx* c = use(ctx);
  if (!out5) return RTGS_E_INVALID;
  memcpy(out5, c->cull.stats, sizeof(c->cull.stats));
  unsigned long long bad = 0;
  if (c->cull.mismatches) HIP_TRY(hipMemcpy(&bad, c->cull.mismatches, sizeof(bad), hipMemcpyDeviceToHost));   // waits for the device
  out5[4] = (int64_t)bad;
  return RTGS_OK;
}
void rtgs_raster_set_bwd_debug(int bits) { rtgs::set_bwd_debug(bits); }
void rtgs_raster_set_bwd_stamps(void* dev) { rtgs::set_bwd_stamps(dev); }
void rtgs_raster_set_fwd_stamps(void* dev) { rtgs::set_fwd_stamps(dev); }
void rtgs_raster_set_onepass_ctx(rtgs_ctx* c, int on) { use(c)->sw.onepass = on != 0; use(c)->plan.valid = false; }
void rtgs_raster_set_fused_sort_ctx(rtgs_ctx* c, int on) { use(c)->sw.fused_sort = on != 0; use(c)->plan.valid = false; }
int rtgs_raster_fused_sort_stats_ctx(rtgs_ctx* ctx, int64_t* out18) {
  rtgs_ctx* c = use(ctx);
  if (!out18) return RTGS_E_INVALID;
  for (int k = 0; k < 3 * FSORT_CLASSES; ++k) out18[k] = 0;
  if (!c->fsort_cls || c->fsort_tiles <= 0) return RTGS_OK;
  std::vector<uint32_t> w((size_t)c->fsort_tiles);
  HIP_TRY(hipMemcpy(w.data(), c->fsort_cls, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));   // waits for the device
  for (uint32_t v : w) {
    if (v == 0xffffffffu) continue;
    const int cls = (int)(v >> 28);
    const int64_t len = (int64_t)(v & 0x0fffffffu);
    if (cls >= FSORT_CLASSES) continue;
    int64_t* o = out18 + 3 * cls;
    o[1] = o[0] == 0 ? len : (len < o[1] ? len : o[1]);
    o[2] = len > o[2] ? len : o[2];
    ++o[0];
  }
  return RTGS_OK;
}
void rtgs_raster_set_tile_gather_ctx(rtgs_ctx* c, int mode) {
  use(c)->sw.tile_gather = (mode >= 0 && mode <= 2) ? mode : 1; use(c)->plan.valid = false; use(c)->gather_blocked = false;
}
int rtgs_raster_tile_gather_stats_ctx(rtgs_ctx* ctx, int64_t* out6) {
  if (!out6) return RTGS_E_INVALID;
  memcpy(out6, use(ctx)->gather_stats, sizeof(use(ctx)->gather_stats));
  out6[4] = GATHER_CHUNK; out6[5] = GATHER_CAND;
  return RTGS_OK;
}
void rtgs_raster_set_bwd_walk_ctx(rtgs_ctx* c, int mode) { use(c)->sw.bwd_walk = (mode >= 1 && mode <= 4) ? mode : 0; }
void rtgs_raster_set_aux_zero_ctx(rtgs_ctx* ctx, void* eight_words) { use(ctx)->aux_zero = (uint32_t*)eight_words; }
int rtgs_raster_last_buffers_ctx(rtgs_ctx* ctx, void** out3) {
  rtgs_ctx* c = use(ctx);
  if (!out3 || !c->last_geom || !c->last_bin || !c->last_img) return RTGS_E_INVALID;
  out3[0] = c->last_geom; out3[1] = c->last_bin; out3[2] = c->last_img;
  return RTGS_OK;
}
int rtgs_raster_backward_buffers(int32_t P, int32_t H, int32_t W, size_t* out) {
  if (!out || P < 0 || H <= 0 || W <= 0) return RTGS_E_INVALID;
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  const GeomLayout G = geom_layout(P, gx, gy, 1);        // budget-independent offsets only
  const ImgLayout I = img_layout(H, W, gx * gy);
  out[0] = G.clamped; out[1] = G.offsets; out[2] = G.slot_count; out[3] = I.bwd_info;
  out[4] = align_up((size_t)(P > 0 ? P : 1) * sizeof(SplatGrad)); out[5] = G.radii; out[6] = G.cull_marks; out[7] = 0;
  return RTGS_OK;
}
int rtgs_raster_image_offsets(int32_t H, int32_t W, size_t* out) {
  if (!out || H <= 0 || W <= 0) return RTGS_E_INVALID;
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  const ImgLayout I = img_layout(H, W, gx * gy);
  out[0] = I.ranges; out[1] = I.n_contrib; out[2] = I.bwd_info; out[3] = I.tile_mode; out[4] = I.total; out[5] = I.depth_pos;
  return RTGS_OK;
}

int rtgs_raster_last_timings_ctx(rtgs_ctx* ctx, float* ms) {
  rtgs_ctx* c = use(ctx);
  if (!ms) return RTGS_E_INVALID;
  for (int i = 0; i < 12; ++i) ms[i] = -1.f;
  if (!c->ev_init) return RTGS_OK;
  // [0] preprocess_fwd(+sat) [1] count+scan of the main pass [2] scatter / emit_keys [3] sort [4] tile_ranges
  // [5] blend_fwd of the main pass [6] blend_bwd (the launches that have lists to walk) [7] preprocess_bwd
  // [8] near slice: hist+count+scan+scatter+sort [9] near slice: blend_fwd [10] grad_reduce [11] unused
  const int pre_end = c->ev_set[EV_SL_BLEND] ? EV_SL_BLEND : EV_PRE;
  const int pairs[11][2] = {{EV_F0, EV_PRE}, {pre_end, EV_SCAN}, {EV_BIN0, EV_EMIT}, {EV_EMIT, EV_SORT},
                            {EV_SORT, EV_RANGES}, {EV_BLEND0, EV_BLEND}, {EV_B0, EV_BWALK}, {EV_BBLEND, EV_BPRE},
                            {EV_PRE, EV_SL_BIN}, {EV_SL_BIN, EV_SL_BLEND}, {EV_BWALK, EV_BBLEND}};
  for (int i = 0; i < 11; ++i) {
    const int a = pairs[i][0], b = pairs[i][1];
    if (!c->ev_set[a] || !c->ev_set[b]) continue;
    if (hipEventSynchronize(c->ev[b]) != hipSuccess) return RTGS_E_HIP;
    float t = 0.f;
    if (hipEventElapsedTime(&t, c->ev[a], c->ev[b]) == hipSuccess) ms[i] = t;
  }
  return RTGS_OK;
}

// ---- the plain entry points: the same calls on the process-wide default context ----------------------------------
int rtgs_raster_forward(const rtgs_raster_settings* s, int32_t P, int32_t M, const float* means3D,
                        const float* opacities, const float* shs, const float* scales, const float* rotations,
                        const float* normal_w, const int32_t* tile_mask, float* out_color, float* out_depth,
                        int32_t* out_cidx, int32_t* out_didx, float* out_cw, float* out_dw, float* out_T,
                        int32_t* out_radii, rtgs_resize_fn geom_resize, void* geom_user,
                        rtgs_resize_fn binning_resize, void* binning_user, rtgs_resize_fn image_resize,
                        void* image_user, int64_t* num_rendered_host, void* stream) {
  return rtgs_raster_forward_ctx(nullptr, s, P, M, means3D, opacities, shs, scales, rotations, normal_w, tile_mask,
                                 out_color, out_depth, out_cidx, out_didx, out_cw, out_dw, out_T, out_radii, geom_resize,
                                 geom_user, binning_resize, binning_user, image_resize, image_user, num_rendered_host, 0, stream);
}
int rtgs_raster_backward(const rtgs_raster_settings* s, int32_t P, int32_t M, int64_t R, const float* means3D,
                         const float* opacities, const float* shs, const float* scales, const float* rotations,
                         const float* normal_w, void* geom_buffer, void* binning_buffer,
                         const void* image_buffer, const float* out_color, const float* out_T, const int32_t* out_didx,
                         const float* dL_dcolor, const float* dL_ddepth, float* dL_dmeans3D, float* dL_dopacities,
                         float* dL_dshs, float* dL_dscales, float* dL_drotations, float* dL_dnormal_w,
                         void* grad_scratch, void* stream) {
  return backward_impl(nullptr, s, P, M, R, means3D, opacities, shs, scales, rotations, normal_w, geom_buffer,
                       binning_buffer, image_buffer, out_color, out_T, out_didx, dL_dcolor, dL_ddepth, dL_dmeans3D,
                       dL_dopacities, dL_dshs, dL_dscales, dL_drotations, dL_dnormal_w, grad_scratch, nullptr, 0, P, stream);
}
int rtgs_raster_backward_rows(const rtgs_raster_settings* s, int32_t P, int32_t M, int64_t R, const float* means3D,
                              const float* opacities, const float* shs, const float* scales, const float* rotations,
                              const float* normal_w, void* geom_buffer, void* binning_buffer,
                              const void* image_buffer, const float* out_color, const float* out_T,
                              const int32_t* out_didx, const float* dL_dcolor, const float* dL_ddepth,
                              float* dL_dmeans3D, float* dL_dopacities, float* dL_dshs, float* dL_dscales,
                              float* dL_drotations, float* dL_dnormal_w, void* grad_scratch, uint8_t* row_state,
                              void* stream) {
  return rtgs_raster_backward_rows_ctx(nullptr, s, P, M, R, means3D, opacities, shs, scales, rotations, normal_w,
                                       geom_buffer, binning_buffer, image_buffer, out_color, out_T, out_didx, dL_dcolor,
                                       dL_ddepth, dL_dmeans3D, dL_dopacities, dL_dshs, dL_dscales, dL_drotations,
                                       dL_dnormal_w, grad_scratch, row_state, stream);
}
int rtgs_raster_last_stats(int64_t* out) { return rtgs_raster_last_stats_ctx(nullptr, out); }
void rtgs_raster_set_counters(void* counters) { rtgs_raster_set_counters_ctx(nullptr, counters); }
void rtgs_raster_set_profiling(int enable) { rtgs_raster_set_profiling_ctx(nullptr, enable); }
void rtgs_raster_set_near_slice(int mode, int budget) { rtgs_raster_set_near_slice_ctx(nullptr, mode, budget); }
int rtgs_raster_last_slice_stats(int64_t* out) { return rtgs_raster_last_slice_stats_ctx(nullptr, out); }
void rtgs_raster_force_sort_path(int enable) { rtgs_raster_force_sort_path_ctx(nullptr, enable); }
int rtgs_raster_last_timings(float* ms) { return rtgs_raster_last_timings_ctx(nullptr, ms); }

}  // extern "C"
