"""The near-slice blend gathers its tile's list itself from row bands (RasterContext.set_tile_gather, include/rtgs_debug.h):
every comparison here is the switch FORCED (2) or AUTOMATIC (1) against OFF (0) - bin_place in front of the blend - on the
same seeded input, through opt.step_slam: only the speculative map step takes the path.

Two runs per arm.  With a zero learning rate every step renders the same map to the bit, so the forward outputs, the slice
statistics (instances included) and the speculation counters must be EQUAL.  With a learning rate the arms differ only in
how the lists were built: losses within 1e-5 relative, parameters frac_bad(., ., 2e-6) < 1e-3 - the bounds of
tests/test_fused_sort_gpu.py::test_map_steps_equal_with_the_switch_on_and_off.

Two cases of the issue cannot be reached through a map step and are not here: a tile whose row band is EMPTY (or holds no entry
over its column) has an empty list, cannot finish inside the slice, and so never stands behind the guess "the slice finishes
every tile" unless it is masked off - and a masked tile does not read its band; a listed row of radius 0 does not exist (the
cull gives a visible row a radius of at least 2, an invisible one is not listed).  The rows of the boundary scene whose thousands of
entries miss all but two columns, and the listed rows below 1/255 opacity, are the nearest reachable cases."""
import pytest
import torch

from rtg_slam_amd import map_optim as mo
from rtg_slam_amd import rasterizer as rz
from rtg_slam_amd import synth
from tests import raster_util as ru

pytestmark = pytest.mark.gpu

CAM = synth.CONFIG2                                               # 640 x 480: 40 x 30 tiles
MID = synth.CameraSpec(272, 400, 300.0, 300.0, 199.5, 135.5)      # 17 x 25 = 425 tiles: the near slice is considered
SIZES = (1, 2, 3, 64, 65, 255, 256, 257, 1023, 1024)
PAD = 100_000                                                     # per-tile segments need the large-map threshold
DEV = "cuda:0"


def _specks(u, v, z, sigma_px, opacity):
    """Isotropic Gaussians of `sigma_px` pixels at pixel (u, v), depth z."""
    n = u.shape[0]
    xyz = torch.stack([(u - CAM.cx) / CAM.fx * z, (v - CAM.cy) / CAM.fy * z, z], 1)
    sc = (sigma_px * z / CAM.fx).reshape(n, 1).expand(n, 3)
    return xyz, sc, torch.full((n, 1), float(opacity))


def _designed_map(sizes=SIZES, boundary=None, discs=0):
    """tests/test_fused_sort_gpu.py's designed map with a backdrop, built here: clusters of faint specks (0.26 px sigma, inside
    their tile) on tiles three apart in tile row 2, three opaque sheets behind everything over all 40 x 30 tiles - every tile
    saturates inside the slice, the finished tiles' lists have exactly the lengths of `sizes` from 64 on (clusters are three
    specks smaller) - and rows behind the camera up to PAD.  Besides: five 4-px specks clipped by each image edge, five each
    with the centre left of and below the image, fifty listed specks below 1/255 opacity.
    `boundary` = (chunk, capacity): six columns of 4-px specks centred 9 px left of tile column 11, in tile rows 7, 16, 22 and
    4, 19, 26 (no other live rect but the sheets touches those rows or their neighbours): their 13-px rects reach column 11
    and the rows above and below, their alpha >= 1/255 extent (7.3 px at opacity 0.02) does not leave column 10, which the
    test masks off.  With the three sheets the bands of those rows and their neighbours hold chunk - 1, chunk, chunk + 1 and
    capacity - 1, capacity, capacity + 1 entries, all of them x-candidates of the tiles in columns 9 and 11, three of them
    hits; every other tile of those rows filters all but the sheets out.
    `discs`: that many thin rotated discs of ru.make_scene(..., r_range=(0.02, 0.12)) in front of the sheets."""
    gen = torch.Generator().manual_seed(21)
    xyz, scales, opacity = [], [], []
    for k, n in enumerate(sizes):
        n = max(n - 3, 0)
        tx, ty = 2 + 3 * k, 2
        u = 16 * tx + 8 + (torch.rand(n, generator=gen) - 0.5) * 4.0
        v = 16 * ty + 8 + (torch.rand(n, generator=gen) - 0.5) * 4.0
        z = torch.full((n,), 0.9 + 0.01 * k) if k % 2 == 1 else 0.9 + 0.2 * torch.rand(n, generator=gen)
        a, b, c = _specks(u, v, z, torch.full((n,), 0.26), 0.02)
        xyz.append(a); scales.append(b); opacity.append(c)
    edge_uv = [(3.0, 200.0), (636.0, 200.0), (300.0, 3.0), (300.0, 476.0), (-5.0, 200.0), (300.0, 484.0)]
    for (u0, v0) in edge_uv:
        u = u0 + torch.rand(5, generator=gen); v = v0 + torch.rand(5, generator=gen)
        a, b, c = _specks(u, v, 1.0 + 0.1 * torch.rand(5, generator=gen), torch.full((5,), 4.0), 0.5)
        xyz.append(a); scales.append(b); opacity.append(c)
    u = 640.0 * torch.rand(50, generator=gen); v = 480.0 * torch.rand(50, generator=gen)
    a, b, c = _specks(u, v, 1.0 + 0.1 * torch.rand(50, generator=gen), torch.full((50,), 2.0), 0.003)
    xyz.append(a); scales.append(b); opacity.append(c)
    if boundary is not None:
        chunk, capacity = boundary
        for row, target in ((7, chunk - 1), (16, chunk), (22, chunk + 1), (4, capacity - 1), (19, capacity), (26, capacity + 1)):
            n = target - 3
            u = torch.full((n,), 16.0 * 11 - 9.0); v = 16.0 * row + 8.0 + (torch.rand(n, generator=gen) - 0.5)
            a, b, c = _specks(u, v, 0.9 + 0.2 * torch.rand(n, generator=gen), torch.full((n,), 4.0), 0.02)
            xyz.append(a); scales.append(b); opacity.append(c)
    xyz = torch.cat(xyz); scales = torch.cat(scales); opacity = torch.cat(opacity)
    perm = torch.randperm(xyz.shape[0], generator=gen)            # shuffled rows: ids neither contiguous nor in placement order
    xyz, scales, opacity = xyz[perm], scales[perm], opacity[perm]
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).expand(xyz.shape[0], 4)
    if discs:
        d, _ = ru.make_scene(discs, CAM, seed=7, r_range=(0.02, 0.12))
        xyz = torch.cat([xyz, d["xyz"]]); scales = torch.cat([scales, d["scales"]]); opacity = torch.cat([opacity, d["opacity"]])
        rot = torch.cat([rot, d["rotations"]])
        far = float(d["xyz"][:, 2].max())
    else:
        far = 1.5
    xyz = torch.cat([xyz, torch.tensor([[0.0, 0.0, far + 0.5], [0.0, 0.0, far + 0.6], [0.0, 0.0, far + 0.7]])])
    scales = torch.cat([scales, torch.tensor([[8.0, 8.0, 0.01]] * 3) * (far + 0.5) / 2.0])
    opacity = torch.cat([opacity, torch.ones(3, 1)])
    rot = torch.cat([rot, torch.tensor([[1.0, 0.0, 0.0, 0.0]]).expand(3, 4)])
    m = PAD - xyz.shape[0]
    assert m > 0
    xyz = torch.cat([xyz, torch.tensor([[0.0, 0.0, -1.0]]).expand(m, 3)])
    scales = torch.cat([scales, torch.full((m, 3), 0.0005)])
    opacity = torch.cat([opacity, torch.full((m, 1), 0.02)])
    rot = torch.cat([rot, torch.tensor([[1.0, 0.0, 0.0, 0.0]]).expand(m, 4)]).contiguous()
    n = xyz.shape[0]
    shs = torch.cat([torch.rand(n, 1, 3, generator=gen) * 2.0, 0.05 * torch.randn(n, 15, 3, generator=gen)], 1)
    g = dict(xyz=xyz.contiguous(), opacity=opacity.contiguous(), scales=scales.contiguous(), rotations=rot, shs=shs.contiguous())
    g["normal"] = synth.normal_from_scale_rot(g["scales"], g["rotations"]).contiguous()
    return g


def _run(g, cam, mode, lr, mask=None, near=(1, 384), steps=5, check=False):
    """`steps` one-call map steps with the switch at `mode`: losses, parameters, the last step's images, the slice statistics,
    and what the speculation, gather and cull-cache counters moved by."""
    ctx = rz.current_context()
    try:
        ctx.set_near_slice(*near)
        ctx.set_tile_gather(mode)
        ctx.set_cull_cache_check(check)
        opt = mo.ShardedMapOptimizer(mo.pack_from_activated({k: v.to(DEV) for k, v in g.items()}), lr_col=mo.default_lr_columns() * lr)
        gen = torch.Generator().manual_seed(3)
        gt_c = torch.rand(3, cam.H, cam.W, generator=gen).to(DEV)
        gt_d = (1.0 + torch.rand(1, cam.H, cam.W, generator=gen)).to(DEV)
        _, s = ru.make_scene(8, cam, seed=1)                      # identity view
        rs = ru.hip_settings(s, DEV)
        b_sp, b_ga, b_cc = ctx.speculation_stats(), ctx.tile_gather_stats(), ctx.cull_cache_stats()
        opt.begin_local_optimization()
        losses = [float(opt.step_slam(rs, gt_c, gt_d, mask)) for _ in range(steps)]
        a_sp, a_ga, a_cc = ctx.speculation_stats(), ctx.tile_gather_stats(), ctx.cull_cache_stats()
        st = ctx.last_stats()
        return dict(losses=losses, params=opt.params.detach().cpu(), images=[t.detach().cpu().clone() for t in opt.last_render],
                    slice=ctx.last_slice_stats(), stats={k: st[k] for k in (0, 2, 3, 5, 6, 7)}, rendered=int(opt.last_num_rendered),
                    spec={k: a_sp[k] - b_sp[k] for k in a_sp},
                    gather={k: a_ga[k] - b_ga[k] for k in ("gathered", "fell_back_listed", "fell_back_longest", "fell_back_layout")},
                    cull={k: a_cc[k] - b_cc[k] for k in a_cc})
    finally:
        ctx.set_cull_cache_check(False)
        ctx.set_tile_gather(1)
        ctx.set_near_slice(2, 384)


def _compare(g, cam, mode, what, **kw):
    """The switch at `mode` against 0; returns the two zero-learning-rate runs."""
    a0, b0 = _run(g, cam, mode, 0.0, **kw), _run(g, cam, 0, 0.0, **kw)
    print("tile gather,", what, dict(slice=a0["slice"], spec=a0["spec"], gather=a0["gather"], spec_off=b0["spec"]))
    assert a0["slice"] == b0["slice"] and a0["stats"] == b0["stats"] and a0["rendered"] == b0["rendered"], (what, a0["slice"], b0["slice"], a0["stats"], b0["stats"])
    for k, (x, y) in enumerate(zip(a0["images"], b0["images"])):
        assert torch.equal(x, y), (what, "image", k)
    for x, y in zip(a0["losses"], b0["losses"]):
        assert abs(x - y) <= 1e-5 * max(1.0, abs(x)), (what, a0["losses"], b0["losses"])
    assert b0["gather"]["gathered"] == 0, (what, b0["gather"])
    a1, b1 = _run(g, cam, mode, 1e-4, **kw), _run(g, cam, 0, 1e-4, **kw)
    assert a1["slice"] == b1["slice"], (what, a1["slice"], b1["slice"])
    for x, y in zip(a1["losses"], b1["losses"]):
        assert abs(x - y) <= 1e-5 * max(1.0, abs(x)), (what, a1["losses"], b1["losses"])
    assert ru.frac_bad(a1["params"], b1["params"], 2e-6) < 1e-3, what
    return a0, b0, a1, b1


def _held(a0, b0, a1, b1, what):
    """Every guess held in both arms, and the forced / automatic arm gathered."""
    for r in (a0, a1):
        assert r["gather"]["gathered"] >= 1 and r["spec"]["failed"] == 0 and r["slice"]["tiles_left_to_pass2"] == 0, (what, r["gather"], r["spec"], r["slice"])
    assert a0["spec"] == b0["spec"] and a1["spec"] == b1["spec"], (what, a0["spec"], b0["spec"], a1["spec"], b1["spec"])


def test_designed_lists_every_length_at_which_the_prologue_takes_another_path():
    """Lists of 1, 2, 3, 64, 65, 255, 256, 257, 1 023 and 1 024 entries, all in one tile row (its band is scanned in two rounds);
    rects over every row and column (the sheets), clipped by each image edge, centred outside the image; listed rows below
    1/255 opacity."""
    _held(*_compare(_designed_map(), CAM, 2, "designed lists"), "designed lists")


def test_a_list_above_the_arena_fails_one_guess_and_keeps_the_path_off():
    """One more cluster of 1 025 entries.  Forced: the first speculative step gathers, that tile counts 1 025 hits and leaves
    itself to pass 2, the guess fails, the step is redone classically - whose verify reports the list, which alone keeps the
    path off: exactly one gathered forward and one failed guess over the run, the later steps fall back for `longest`.
    Ends equal to switch 0, which never fails (the launch in front of the blend sorts 1 025 entries)."""
    g = _designed_map(sizes=SIZES + (1025,))
    a0, b0, a1, b1 = _compare(g, CAM, 2, "1 025 entries")
    for r in (a0, a1):
        assert r["gather"]["gathered"] == 1 and r["spec"]["failed"] == 1 and r["gather"]["fell_back_longest"] >= 1, (r["gather"], r["spec"])
        assert r["slice"]["tiles_left_to_pass2"] == 0, r["slice"]
    for r in (b0, b1):
        assert r["spec"]["failed"] == 0 and r["spec"]["speculative"] >= 1, r["spec"]


def test_band_and_candidate_boundaries():
    """Bands of chunk - 1, chunk, chunk + 1 and capacity - 1, capacity, capacity + 1 entries (both constants from the stats
    call), every entry an x-candidate of two tiles and three of them hits; in the other tiles of those rows all but the
    sheets miss the column filter."""
    st = rz.current_context().tile_gather_stats()
    g = _designed_map(boundary=(st["chunk"], st["capacity"]))
    mask = torch.ones(30, 40, dtype=torch.int32)
    for row in (7, 16, 22, 4, 19, 26):
        mask[row, 10] = 0
    _held(*_compare(g, CAM, 2, "boundaries", mask=mask), "boundaries")


@pytest.mark.parametrize("shape", ["random", "band"])
def test_tile_masks(shape):
    """A 70 % random tile mask, and a band of tile rows - the tile-band mode of the multi-GPU step - over thin rotated discs
    whose rects hold tiles tile_visible rejects."""
    g = _designed_map(sizes=SIZES[:8], discs=1500)      # (no list near 1 024 entries: the discs land on the clusters' tiles too)
    if shape == "random":
        mask = (torch.rand(30, 40, generator=torch.Generator().manual_seed(4)) < 0.7).int()
    else:
        mask = torch.zeros(30, 40, dtype=torch.int32)
        mask[9:21] = 1
    _held(*_compare(g, CAM, 2, "mask " + shape, mask=mask), "mask " + shape)


def test_automatic_mode_takes_the_path_on_a_depth_complex_map():
    """The 150 000-Gaussian scene of the fused-sort test, switch at its default."""
    g, _ = ru.make_scene(150_000, MID, seed=6)
    _held(*_compare(g, MID, 1, "automatic", near=(2, 384), steps=4), "automatic")


def test_a_declined_slice_runs_what_it_ran():
    """A surface-shaped map declines the slice (kind 2): nothing gathers, nothing falls back, and the forward leaves the
    statistics of tests/test_speculation_gpu.py::test_every_forward_path_leaves_the_same_statistics, equal with the switch
    at 1 and at 0."""
    g = synth.surface_gaussians(150_000, MID, seed=5)
    _run(g, MID, 0, 0.0, near=(2, 384), steps=2)      # (the context learns that this map declines: both arms start alike)
    a0, b0 = _run(g, MID, 1, 0.0, near=(2, 384), steps=4), _run(g, MID, 0, 0.0, near=(2, 384), steps=4)
    print("tile gather, declined:", a0["slice"], a0["spec"], a0["gather"])
    assert a0["gather"] == dict(gathered=0, fell_back_listed=0, fell_back_longest=0, fell_back_layout=0), a0["gather"]
    assert a0["spec"] == b0["spec"] and a0["spec"]["speculative"] >= 1 and a0["spec"]["failed"] == 0, (a0["spec"], b0["spec"])
    assert (a0["stats"], a0["slice"], a0["rendered"]) == (b0["stats"], b0["slice"], b0["rendered"])
    for x, y in zip(a0["images"], b0["images"]):
        assert torch.equal(x, y)


def test_same_view_steps_with_the_cull_cache_check_on():
    """The path sits behind cull-cache hits: six same-view steps with the cache's self-check on."""
    g = _designed_map()
    r = _run(g, CAM, 2, 1e-4, steps=6, check=True)
    print("tile gather, cull-cache check:", r["cull"], r["gather"], r["spec"])
    assert r["gather"]["gathered"] >= 2 and r["spec"]["failed"] == 0, (r["gather"], r["spec"])
    assert r["cull"]["hits"] >= 1 and r["cull"]["check_mismatches"] == 0, r["cull"]
