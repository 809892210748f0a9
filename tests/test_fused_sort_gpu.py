"""The near-slice blend sorts its tile's list itself (RasterContext.set_fused_sort, include/rtgs_debug.h): every
comparison here is the switch ON against OFF - the sort launches in front of the blend - on the same seeded input.
The order of a tile list is total (depth bits, then Gaussian id), so forward outputs must be bit-equal and slice
statistics equal; gradients are float-atomic sums and get the bound test_onepass_binning_is_bit_identical uses
(1e-4 of the tensor's maximum, frac_bad < 1e-3)."""
import pytest
import torch

from rtg_slam_amd import map_optim as mo
from rtg_slam_amd import rasterizer as rz
from rtg_slam_amd import synth
from tests import raster_util as ru

pytestmark = pytest.mark.gpu

CAM = synth.CONFIG2                                               # 640 x 480: 40 x 30 tiles
SIZES = (1, 2, 3, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3071, 3072, 3073)
MIXED = 700                                                       # one more cluster: runs of equal depths


def _designed_map(pad_to=0, backdrop=False):
    """Clusters of faint specks, each on a tile of its own (tiles three apart; centre jitter <= 2 px; 0.26 px sigma, so the
    3-sigma radius is 2 px: every speck's rect and extent stay inside its tile).  Cluster k of SIZES: odd k = every speck at
    one bit-equal depth (the order is by id, through the tie fix-up), even k = distinct random depths; the last cluster
    mixes runs of equal depths.  `backdrop`: three opaque sheets behind everything, over the whole image - every tile then
    saturates INSIDE the slice, so the blend's outputs and the backward's walk come from the slice's lists; the clusters
    are three specks smaller there (none for sizes 1 to 3), so the finished tiles' lists have exactly the lengths of SIZES
    from 64 on: the outputs depend on the order at 255, 256, 257, 1 023 and 1 024 entries.  `pad_to`: rows behind the
    camera up to that many Gaussians (per-tile segments need 100 000)."""
    gen = torch.Generator().manual_seed(21)
    xyz, sizes = [], SIZES + (MIXED,)
    for k, n in enumerate(sizes):
        if backdrop:
            n = max(n - 3, 0)
        tx, ty = 2 + 3 * (k % 12), 2 + 3 * (k // 12)
        u = 16 * tx + 8 + (torch.rand(n, generator=gen) - 0.5) * 4.0
        v = 16 * ty + 8 + (torch.rand(n, generator=gen) - 0.5) * 4.0
        if k == len(SIZES):
            z = 0.9 + 0.01 * torch.randint(0, 8, (n,), generator=gen).float()
        elif k % 2 == 1:
            z = torch.full((n,), 0.9 + 0.01 * k)
        else:
            z = 0.9 + 0.2 * torch.rand(n, generator=gen)
        xyz.append(torch.stack([(u - CAM.cx) / CAM.fx * z, (v - CAM.cy) / CAM.fy * z, z], 1))
    xyz = torch.cat(xyz)
    # shuffled rows: a cluster's ids are neither contiguous nor in placement order
    xyz = xyz[torch.randperm(xyz.shape[0], generator=gen)]
    n = xyz.shape[0]
    scales = torch.full((n, 3), 0.0005)
    opacity = torch.full((n, 1), 0.02)
    if backdrop:
        xyz = torch.cat([xyz, torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, 2.1], [0.0, 0.0, 2.2]])])
        scales = torch.cat([scales, torch.tensor([[8.0, 8.0, 0.01]] * 3)])
        opacity = torch.cat([opacity, torch.ones(3, 1)])
    if pad_to > xyz.shape[0]:
        m = pad_to - xyz.shape[0]
        xyz = torch.cat([xyz, torch.tensor([[0.0, 0.0, -1.0]]).expand(m, 3)])
        scales = torch.cat([scales, torch.full((m, 3), 0.0005)])
        opacity = torch.cat([opacity, torch.full((m, 1), 0.02)])
    n = xyz.shape[0]
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).expand(n, 4).contiguous()
    shs = torch.cat([torch.rand(n, 1, 3, generator=gen) * 2.0, 0.05 * torch.randn(n, 15, 3, generator=gen)], 1)
    g = dict(xyz=xyz.contiguous(), opacity=opacity, scales=scales, rotations=rot, shs=shs.contiguous())
    g["normal"] = synth.normal_from_scale_rot(g["scales"], g["rotations"]).contiguous()
    _, s = ru.make_scene(8, CAM, seed=1)                        # identity view
    return g, s


def _grads(cam, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(3, cam.H, cam.W, generator=gen), torch.randn(1, cam.H, cam.W, generator=gen)


def _on_off(s, g, mask, grads, mode, budget, with_stats=False):
    """{True, False} -> (outputs, gradients, slice statistics), and the class statistics of a fused run with counters."""
    ctx = rz.current_context()
    res, cls = {}, None
    try:
        ctx.set_near_slice(mode, budget)
        for on in (True, False):
            ctx.set_fused_sort(on)
            out, gd = ru.hip_run(s, g, tile_mask=mask, grads=grads)
            res[on] = (out, gd, ctx.last_slice_stats())
        if with_stats:
            ctx.set_fused_sort(True)
            ntiles = ((s.image_height + 15) // 16) * ((s.image_width + 15) // 16)
            counters = torch.zeros(2 * ntiles, dtype=torch.int64, device="cuda:0")
            ctx.set_counters(counters)
            try:
                out, gd = ru.hip_run(s, g, tile_mask=mask, grads=grads)
                cls = ctx.fused_sort_stats()
            finally:
                ctx.set_counters(None)
            res["counted"] = (out, gd, ctx.last_slice_stats())
    finally:
        ctx.set_fused_sort(True)
        ctx.set_near_slice(2, 384)
    return res, cls


def _assert_same(a, b, what):
    (out_a, gd_a, st_a), (out_b, gd_b, st_b) = a, b
    assert st_a == st_b, (what, st_a, st_b)
    for k, (x, y) in enumerate(zip(out_a, out_b)):
        assert torch.equal(x, y), (what, k, st_a)
    for k in ru.FIELDS:
        scale = float(gd_a[k].abs().max()) + 1e-12
        assert ru.frac_bad(gd_b[k], gd_a[k], 1e-4 * scale) < 1e-3, (what, k, st_a)


@pytest.mark.parametrize("backdrop", [False, True])
@pytest.mark.parametrize("pad_to", [0, 100_000])
def test_designed_lists_every_class_and_boundary(pad_to, backdrop):
    """One tile list of every length at which the prologue takes another path, with P below the one-pass threshold (count /
    scan / scatter placement, ranges from the scan) and padded above it (per-tile segments, ranges from the counts)."""
    g, s = _designed_map(pad_to, backdrop)
    res, cls = _on_off(s, g, None, _grads(CAM), 1, 384, with_stats=True)
    print("fused sort classes:", dict(pad_to=pad_to, backdrop=backdrop, slice=res[True][2]), cls)
    _assert_same(res[True], res[False], "on/off")
    _assert_same(res["counted"], res[False], "counted/off")
    assert res[True][2]["used"] == 1
    entered = ("bitonic", "radix", "launch", "pass2") + (() if backdrop else ("empty", "single"))
    assert all(cls[k]["tiles"] > 0 for k in entered), cls
    assert sum(c["tiles"] for c in cls.values()) == 40 * 30, cls
    if not backdrop:
        assert cls["empty"]["tiles"] == 40 * 30 - len(SIZES) - 1 and cls["single"]["tiles"] == 1, cls
        assert (cls["bitonic"]["tiles"], cls["bitonic"]["shortest"], cls["bitonic"]["longest"]) == (6, 2, 256), cls
        assert (cls["radix"]["tiles"], cls["radix"]["shortest"], cls["radix"]["longest"]) == (4, 257, 1024), cls
        assert (cls["launch"]["tiles"], cls["launch"]["shortest"], cls["launch"]["longest"]) == (3, 1025, 3072), cls
        assert (cls["pass2"]["tiles"], cls["pass2"]["shortest"]) == (1, 3073), cls
        assert res[True][2]["tiles_left_to_pass2"] >= 1
    else:
        # the sheets lie on every tile (three entries where there is no cluster, or one of size 1 to 3); the others carry
        # exactly the designed lengths
        assert (cls["bitonic"]["tiles"], cls["bitonic"]["shortest"], cls["bitonic"]["longest"]) == (40 * 30 - 8, 3, 256), cls
        assert (cls["radix"]["tiles"], cls["radix"]["shortest"], cls["radix"]["longest"]) == (4, 257, 1024), cls
        assert (cls["launch"]["tiles"], cls["launch"]["shortest"], cls["launch"]["longest"]) == (3, 1025, 3072), cls
        assert (cls["pass2"]["tiles"], cls["pass2"]["shortest"]) == (1, 3073), cls
        # the sheets finish every tile whose list was sorted: the outputs compared above came from the slice's lists
        assert res[True][2]["tiles_finished"] == 40 * 30 - cls["pass2"]["tiles"], (res[True][2], cls)


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_random_scene(masked, forced):
    """The scene of test_onepass_binning_is_bit_identical in automatic slice mode, with and without a 70 % random tile mask;
    and - `forced` - its larger discs with the slice forced, where the slice holds every tile's list and finishes tiles."""
    g, s = ru.make_scene(120_000, CAM, seed=7, pose_seed=2, **(dict(r_range=(0.02, 0.12)) if forced else {}))
    mask = None
    if masked:
        mask = (torch.rand(30, 40, generator=torch.Generator().manual_seed(4)) < 0.7).int()
    res, _ = _on_off(s, g, mask, _grads(CAM), 1 if forced else 2, 384)
    print("fused sort, random scene:", dict(masked=masked, forced=forced, slice=res[True][2]))
    _assert_same(res[True], res[False], "on/off")
    assert res[True][2]["used"] == 1, res[True][2]
    if forced:
        assert res[True][2]["instances"] > 0 and res[True][2]["tiles_finished"] > 0, res[True][2]


MID = synth.CameraSpec(272, 400, 300.0, 300.0, 199.5, 135.5)      # 17 x 25 = 425 tiles: the near slice is considered


def _steps(g, cam, fused, steps=4, lr=1e-4):
    dev = "cuda:0"
    ctx = rz.current_context()
    ctx.set_fused_sort(fused)
    try:
        packed = mo.pack_from_activated({k: v.to(dev) for k, v in g.items()})
        opt = mo.ShardedMapOptimizer(packed, lr_col=mo.default_lr_columns() * lr)
        gen = torch.Generator().manual_seed(3)
        gt_c = torch.rand(3, cam.H, cam.W, generator=gen).to(dev)
        gt_d = (1.0 + torch.rand(1, cam.H, cam.W, generator=gen)).to(dev)
        _, s = ru.make_scene(8, cam, seed=1)
        rs = ru.hip_settings(s, dev)
        before = ctx.speculation_stats()
        opt.begin_local_optimization()
        losses = [float(opt.step_slam(rs, gt_c, gt_d, None)) for _ in range(steps)]
        after = ctx.speculation_stats()
        return losses, opt.params.detach().cpu(), ctx.last_slice_stats(), {k: after[k] - before[k] for k in after}
    finally:
        ctx.set_fused_sort(True)


def test_map_steps_equal_with_the_switch_on_and_off():
    """Four one-call map steps (speculation on) on a depth-complex map that takes the slice: losses and parameters as
    tests/test_speculation_gpu.py compares them."""
    g, _ = ru.make_scene(150_000, MID, seed=6)
    la, pa, sa, spa = _steps(g, MID, True)
    lb, pb, sb, spb = _steps(g, MID, False)
    print("fused sort, map steps:", sa, la, spa, spb)
    assert sa == sb and sa["used"] == 1 and sa["tiles_left_to_pass2"] == 0, (sa, sb)
    # the first step(s) build the history; the rest guess "the slice finishes every tile" (the speculative call site), and hold
    assert spa == spb and spa["speculative"] >= 1 and spa["failed"] == 0, (spa, spb)
    for x, y in zip(la, lb):
        assert abs(x - y) <= 1e-5 * max(1.0, abs(x)), (la, lb)
    assert ru.frac_bad(pa, pb, 2e-6) < 1e-3
