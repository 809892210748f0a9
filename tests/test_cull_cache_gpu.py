"""The cull cache of the one-call map step (include/rtgs_raster.h: rtgs_raster_set_cull_cache_ctx): on a view that stays,
the forward re-culls only the rows the last tail stepped (recull_rows) instead of culling the whole map and rebuilding
the depth histograms.

* wherever the cache is on, its self-check is on too: every hit also runs the full cull + slice_hist into scratch copies
  and compares all seven arrays word for word on the device; `check_mismatches` stays 0 after every step;
* the same sequence of steps with the cache on and off gives the same losses and parameters (bounds of
  test_speculation_gpu._same: gradient-slot order is the only run-to-run difference);
* everything that may change a row's cull result, the view or the buffers makes the next step cull the whole map."""
import ctypes as C
import functools

import pytest
import torch

from rtg_slam_amd import _lib
from rtg_slam_amd import map_optim as mo
from rtg_slam_amd import rasterizer as rz
from rtg_slam_amd import synth
from tests import raster_util as ru

pytestmark = pytest.mark.gpu

MID = synth.CameraSpec(272, 400, 300.0, 300.0, 199.5, 135.5)      # 17 x 25 = 425 tiles: the near slice is considered
OTHER = synth.CameraSpec(288, 416, 300.0, 300.0, 207.5, 143.5)    # another image size (18 x 26 tiles)
N = 150_000                                                       # just over the large-map size (100 000)
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _scene(kind):
    """kind 2: a single-layer map, the kernels decline the slice (single pass over the visible list);
    kind 1: a depth-complex volume, the slice finishes every tile (bench.py's headline structure)."""
    if kind == 2:
        return synth.surface_gaussians(N, MID, seed=5)
    # (discs twice the default size: at half the headline's focal length they cover the pixels as often as on the headline map,
    # so that every pixel saturates inside the slice)
    return ru.make_scene(N, MID, seed=6, r_range=(0.002, 0.1))[0]


@functools.lru_cache(maxsize=None)
def _gt(cam):
    gen = torch.Generator().manual_seed(3)
    return torch.rand(3, cam.H, cam.W, generator=gen).to(DEV), (1.0 + torch.rand(1, cam.H, cam.W, generator=gen)).to(DEV)


def _settings(cam, pose):
    _, s = ru.make_scene(8, cam, seed=1, pose_seed=pose)
    return ru.hip_settings(s, DEV)


def _marks(opt, cam):
    """The mark bytes the last tail left in the geometry buffer (one per row of the rendered map)."""
    off = (C.c_size_t * 8)()
    P = opt._active()[0]
    _lib.check(_lib.load().rtgs_raster_backward_buffers(P, cam.H, cam.W, off), "rtgs_raster_backward_buffers")
    geom = opt._slam_ws["arenas"][0].tensor
    return geom[int(off[6]):int(off[6]) + P].clone()


def _run(kind, cache, steps=12, fresh_settings=False, events=None, n_frozen=0, tail_mode=0, masks=(None,), poses=None,
         watch_marks=False, lr=1e-4, _forced=False):
    """`steps` map iterations; events = {step index: name} applied BEFORE that step.  Returns (losses, parameters, the
    cull-cache counters of the run, live counts, extras)."""
    ctx = rz.current_context()
    g = _scene(kind)
    if poses is None:
        # the volume fills the frustum of the identity view: from there every tile saturates inside the slice (from another
        # pose a third of the image looks past the volume and its tiles stay unfinished); the surface map is seen from pose 1
        poses = (None,) if kind == 1 else (1,)
    ctx.set_cull_cache(cache)
    ctx.set_cull_cache_check(cache)
    try:
        before = ctx.cull_cache_stats()
        packed = mo.pack_from_activated({k: v.to(DEV) for k, v in g.items()})
        opt = mo.ShardedMapOptimizer(packed, lr_col=mo.default_lr_columns() * lr, n_frozen=n_frozen, capacity=N + 4096)
        opt.tail_mode = tail_mode
        cam = MID
        keep = [_settings(cam, poses[0])]
        losses, extras = [], dict(hits_at_event=None, marks_frozen=0, marks_train=0)
        opt.begin_local_optimization()
        for k in range(steps):
            ev = (events or {}).get(k)
            pose = poses[k % len(poses)]
            if ev is not None:
                extras["hits_at_event"] = ctx.cull_cache_stats()["hits"] - before["hits"]
            if ev == "pose":
                poses = (3,)
                pose = 3
                keep.append(_settings(cam, pose))
            elif ev == "view_inplace":                     # the SAME device tensors, rewritten: only the device can notice
                other = _settings(cam, 3)
                keep[-1].viewmatrix.copy_(other.viewmatrix)
                keep[-1].projmatrix.copy_(other.projmatrix)
                keep[-1].campos.copy_(other.campos)
            elif ev == "append":
                opt.append_rows(packed[:300].clone())
            elif ev == "remove":
                m = torch.zeros(opt.N, dtype=torch.bool, device=DEV)
                m[opt.n_frozen + 5:opt.n_frozen + 4000:7] = True
                opt.remove_rows(m, start=opt.n_frozen)
            elif ev == "freeze":
                m = torch.zeros(opt.N, dtype=torch.bool, device=DEV)
                m[opt.n_frozen + 3:opt.n_frozen + 6000:5] = True
                opt.freeze_rows(m)
            elif ev == "image_size":
                cam = OTHER
                keep.append(_settings(cam, pose))
            elif ev == "image_size_back":
                cam = MID
                keep.append(_settings(cam, pose))
            elif ev == "plain_render":
                from rtg_slam_amd.rasterizer import GaussianRasterizer
                gd = {k: v.to(DEV) for k, v in g.items()}
                gy, gx = (cam.H + 15) // 16, (cam.W + 15) // 16
                with torch.no_grad():
                    GaussianRasterizer(keep[-1])(means3D=gd["xyz"], opacities=gd["opacity"], shs=gd["shs"], scales=gd["scales"],
                                                 rotations=gd["rotations"], normal_w=gd["normal"],
                                                 tile_mask=torch.ones(gy, gx, dtype=torch.int32, device=DEV))
            elif ev == "begin_local":
                opt.begin_local_optimization()
            if fresh_settings and k > 0:
                keep.append(_settings(cam, pose))          # the earlier objects stay alive: no address is handed out twice
            gt_c, gt_d = _gt(cam)
            m = masks[k % len(masks)]
            losses.append(float(opt.step_slam(keep[-1], gt_c, gt_d, None if m is None else m.to(DEV))))
            if kind == 1 and k == 1 and not _forced:
                st = ctx.last_slice_stats()
                if not (st["used"] == 1 and st["tiles_left_to_pass2"] == 0):
                    # automatic mode does not take the slice to the end on this map: force it (mode 1) with a budget that
                    # holds every Gaussian of a tile, and start over
                    ctx.set_near_slice(1, 1024)
                    try:
                        return _run(kind, cache, steps, fresh_settings, events, n_frozen, tail_mode, masks, poses, watch_marks, lr, True)
                    finally:
                        ctx.set_near_slice(2, 384)
            if cache:
                assert ctx.cull_cache_stats()["check_mismatches"] == before["check_mismatches"], (k, ev)
            if watch_marks and _lib.load().rtgs_raster_cull_marks_ctx(ctx.ptr):      # armed: the tail of this step marked
                mk = _marks(opt, cam)
                extras["marks_frozen"] += int(mk[:opt.n_frozen].ne(0).sum())
                extras["marks_train"] += int(mk[opt.n_frozen:].ne(0).sum())
        if kind == 1:
            st = ctx.last_slice_stats()
            assert st["used"] == 1 and st["tiles_left_to_pass2"] == 0, st      # else: not the structure this test is about
        after = ctx.cull_cache_stats()
        stats = {k: after[k] - before[k] for k in after}
        print(f"kind {kind} cache {cache} events {events}: {stats} live_counts {opt.live_counts.tolist()} extras {extras}")
        return losses, opt.params.detach().cpu(), stats, opt.live_counts.cpu().tolist(), extras
    finally:
        ctx.set_cull_cache(True)
        ctx.set_cull_cache_check(False)


def _same(a, b):
    """The bounds of tests/test_speculation_gpu.py: _same()."""
    for x, y in zip(a[0], b[0]):
        assert abs(x - y) <= 1e-5 * max(1.0, abs(x)), (a[0], b[0])
    assert ru.frac_bad(a[1], b[1], 2e-6) < 1e-3


@functools.lru_cache(maxsize=None)
def _off_pair(kind):
    """Two runs with the cache off: the reference of cases 1 and 2, and the run-to-run slack of the live counts."""
    return _run(kind, False), _run(kind, False)


def _live_counts_agree(on, off_a, off_b):
    # rows with gradient / rows stepped, summed over the run: a gradient that is exactly zero in one slot order and not in
    # another moves them, so the band is what two cache-off runs span, widened by their own difference on either side
    for c in range(2):
        slack = abs(off_a[3][c] - off_b[3][c])
        lo, hi = min(off_a[3][c], off_b[3][c]) - slack, max(off_a[3][c], off_b[3][c]) + slack
        assert lo <= on[3][c] <= hi, (c, on[3], off_a[3], off_b[3])


@pytest.mark.parametrize("kind", [1, 2])
def test_same_view_steps_hit_and_equal_the_full_cull(kind):
    """Twelve steps with ONE settings object: the first builds the speculation history, the second culls the whole map and
    arms the cache, the rest hit."""
    off_a, off_b = _off_pair(kind)
    on = _run(kind, True)
    assert off_a[2]["hits"] == 0 and off_a[2]["full"] == 0, off_a[2]
    assert on[2]["hits"] >= 9, on[2]
    assert on[2]["check_mismatches"] == 0
    _same(on, off_a)
    _live_counts_agree(on, off_a, off_b)


@pytest.mark.parametrize("kind", [1, 2])
def test_a_fresh_settings_object_per_step_never_hits(kind):
    """The view matrix lives at another address every step: the host sees it, a miss without a redo."""
    off_a, _ = _off_pair(kind)
    on = _run(kind, True, fresh_settings=True)
    assert on[2]["hits"] == 0 and on[2]["view_redos"] == 0, on[2]
    _same(on, off_a)


EVENTS = ["pose", "view_inplace", "append", "remove", "freeze", "image_size", "plain_render", "begin_local", "mask_jump"]


@pytest.mark.parametrize("event", EVENTS)
def test_invalidation_between_two_hit_steps(event):
    """The steps before the event hit (from the fourth on: two learn the slice's decision, one arms the cache); the event
    comes before step 7; the steps after it hit again.  Results are those of the
    same sequence with the cache off, and the self-check never sees a difference."""
    kind, steps = 2, 14
    kw = dict(steps=steps, events={7: event})
    if event == "image_size":
        kw["events"] = {7: "image_size", 8: "image_size_back"}
    if event == "mask_jump":
        # the tile-mask jump of test_a_failed_guess_changes_nothing_and_is_redone: count + scan + scatter sizes one buffer by
        # the guessed total, the jump to the full mask overruns it and the step is redone plainly
        gy, gx = (MID.H + 15) // 16, (MID.W + 15) // 16
        few = (torch.rand(gy, gx, generator=torch.Generator().manual_seed(10)) < 0.15).int()
        kw = dict(steps=steps, masks=(few,) * 7 + (None,) + (few,) * 5 + (None,))
    ctx = rz.current_context()
    if event == "mask_jump":
        ctx.set_onepass(False)
    try:
        spec0 = ctx.speculation_stats()
        on = _run(kind, True, **kw)
        spec1 = ctx.speculation_stats()
        off = _run(kind, False, **kw)
    finally:
        ctx.set_onepass(True)
    _same(on, off)
    st, ex = on[2], on[4]
    assert st["check_mismatches"] == 0
    if event == "mask_jump":
        assert spec1["failed"] - spec0["failed"] >= 1       # the guess failed, the redo culled the whole map ...
        assert st["disarmed"] >= 1 and st["hits"] >= 4, st  # ... and dropped the cache, which came back
        return
    assert ex["hits_at_event"] >= 3, (st, ex)               # hit steps before the event ...
    assert st["hits"] - ex["hits_at_event"] >= 3, (st, ex)  # ... and after it
    if event == "begin_local":
        assert st["hits"] >= 10, st                         # rows unchanged: the cache stays
    else:
        assert st["full"] >= 2, st                          # the step after the event culled the whole map again
    if event == "view_inplace":
        assert st["view_redos"] >= 1, st
    else:
        assert st["view_redos"] == 0, st
    if event == "plain_render":
        assert st["disarmed"] >= 1, st


def test_frozen_rows_are_never_marked():
    """80 % of the rows frozen (the small-map form of the fused tail steps the rest): hits, and only trainable rows are marked."""
    nf = N * 8 // 10
    for kind in (1, 2):
        on = _run(kind, True, n_frozen=nf, watch_marks=True)
        off = _run(kind, False, n_frozen=nf)
        _same(on, off)
        assert on[2]["hits"] >= 9 and on[2]["check_mismatches"] == 0, on[2]
        assert on[4]["marks_frozen"] == 0 and on[4]["marks_train"] > 0, on[4]


@pytest.mark.parametrize("form", ["three_kernel", "small_fused"])
def test_every_tail_form_marks_what_it_steps(form):
    """tail_mode 1 (grad_reduce, preprocess_bwd, rtgs_map_tail_rows) and the fused tail's form for small trainable sets
    (map_fused_tail_kernel<64, 16>: at most 65 536 trainable rows): a tail that forgot a mark would leave a stale row, which
    the self-check counts."""
    kw = dict(tail_mode=1) if form == "three_kernel" else dict(n_frozen=N - 20_000)
    for kind in (1, 2):
        on = _run(kind, True, watch_marks=True, **kw)
        off = _run(kind, False, **kw)
        _same(on, off)
        assert on[2]["hits"] >= 9 and on[2]["check_mismatches"] == 0, on[2]
        assert on[4]["marks_train"] > 0 and on[4]["marks_frozen"] == 0, on[4]
