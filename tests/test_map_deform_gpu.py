"""rtgs_map_deform (csrc/map_deform.hip) against its definition tests/map_deform_reference.py, bit for bit; the render of a deformed
map at the moved pose against the render before; MapOptimizer.deform_rows and what it invalidates."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import pose_graph as pg
from rtg_slam_amd import synth
from rtg_slam_amd.rgbd_align import se3_exp
from tests import map_deform_reference as mdr
from tests import raster_util as ru
from tests.test_map_deform_cpu import DELTA_A, DELTA_B, rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
KEYFRAMES, N_FRAMES = [0, 5, 12], 20


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def table_of_a_closure():
    """Twenty frames, keyframes 0 (held: the identity), 5 and 12: rows on keyframes, between them and after the last."""
    old = [np.eye(4), se3_exp([0, 0.2, 0, 0.3, 0, 0.1]), se3_exp([0, 0.5, 0, 0.6, 0.1, 0.2])]
    new = [old[0], DELTA_A @ old[1], DELTA_B @ old[2]]
    return lc.deform_table(lc.frame_corrections(KEYFRAMES, old, new, N_FRAMES))


def run_kernel(xyz, raw8, tick, table):
    from rtg_slam_amd import _lib
    lib = _lib.load()
    x, r = torch.from_numpy(xyz.copy()).to(DEV), torch.from_numpy(raw8.copy()).to(DEV)
    t, tb = torch.from_numpy(np.ascontiguousarray(tick)).to(DEV), torch.from_numpy(np.ascontiguousarray(table)).to(DEV)
    kind = {torch.int32: 0, torch.int64: 1}[t.dtype]
    rc = lib.rtgs_map_deform(_lib.ptr(x), _lib.ptr(r), _lib.ptr(t), kind, x.shape[0], _lib.ptr(tb), tb.shape[0], _lib.stream(DEV))
    assert rc == 0
    return x.cpu().numpy(), r.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_bit_equal_to_the_definition(n, dtype):
    xyz, raw8 = rows(n, seed=n)
    rng = np.random.default_rng(n + 1)
    tick = rng.integers(-3, N_FRAMES + 6, size=n)                                # below 0 .. beyond the table
    pin = np.array([-2, 0, 5, 12, 3, 8, 15, 19, 20, 24, 2 ** 31 - 1 if dtype == np.int32 else 2 ** 40, -2 ** 31])
    tick[:min(n, pin.size)] = pin[:n] if n < pin.size else pin
    if n == 1:
        tick[0] = 8
    tick = tick.astype(dtype)
    table = table_of_a_closure()
    want_x, want_r = mdr.deform(xyz, raw8, tick, table)
    got_x, got_r = run_kernel(xyz, raw8, tick, table)
    assert np.array_equal(bits(got_x), bits(want_x)) and np.array_equal(bits(got_r), bits(want_r))
    if n >= 63:
        held = np.clip(tick.astype(np.int64), 0, N_FRAMES - 1) == 0
        assert held.any() and (~held).any()
        assert np.array_equal(bits(got_x[held]), bits(xyz[held])) and not np.array_equal(bits(got_x[~held]), bits(xyz[~held]))
    again_x, again_r = run_kernel(xyz, raw8, tick, table)                        # two runs are bit-equal
    assert np.array_equal(bits(again_x), bits(got_x)) and np.array_equal(bits(again_r), bits(got_r))


def test_identity_rows_are_not_written_and_refusals_launch_nothing():
    from rtg_slam_amd import _lib
    lib = _lib.load()
    xyz, raw8 = rows(300, seed=9)
    xyz[::3, 1] = -0.0                                                           # R x + t would make these +0.0
    xyz[1::3] = -0.0
    raw8[::4, 5] = -0.0
    raw8[2::5, 4:8] = (-0.0, -0.0, 1.0, -0.0)
    table = table_of_a_closure()
    table[7] = mdr.IDENTITY_ROW
    table[7, 1] = -0.0                                                           # compares equal to the identity's zero
    tick = np.where(np.arange(300) % 2 == 0, 7, -1).astype(np.int32)             # frame 7's identity, and frame 0's
    got_x, got_r = run_kernel(xyz, raw8, tick, table)
    assert np.array_equal(bits(got_x), bits(xyz)) and np.array_equal(bits(got_r), bits(raw8))
    tick[:] = 9
    got_x, got_r = run_kernel(xyz, raw8, tick, table)
    assert not np.array_equal(bits(got_x[1::3]), bits(xyz[1::3]))                # the same rows ARE written once the row is not
    assert np.array_equal(bits(got_r[:, :4]), bits(raw8[:, :4]))                 # opacity and scales never
    E = _lib.CONSTANTS["RTGS_E_INVALID"]
    x, r = torch.from_numpy(xyz).to(DEV), torch.from_numpy(raw8).to(DEV)
    t, tb = torch.from_numpy(tick).to(DEV), torch.from_numpy(table).to(DEV)
    p, st = _lib.ptr, _lib.stream(DEV)
    good = [p(x), p(r), p(t), 0, 300, p(tb), N_FRAMES, st]
    for i, v in ((0, None), (1, None), (2, None), (5, None), (3, 2), (3, -1), (4, -1), (6, 0), (6, -4),
                 (1, r.data_ptr() + 4), (5, tb.data_ptr() + 8)):
        bad = list(good)
        bad[i] = v
        assert lib.rtgs_map_deform(*bad) == E, (i, v)
    empty = list(good)
    empty[4] = 0
    assert lib.rtgs_map_deform(*empty) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(x.cpu().numpy()), bits(xyz)) and np.array_equal(bits(r.cpu().numpy()), bits(raw8))


# ---- render equivalence ----

CAM = synth.CameraSpec(120, 160, 100.0, 100.0, 79.5, 59.5)
DELTA = se3_exp(np.concatenate([np.deg2rad(3.0) * np.array([0.6, 0.64, -0.48]), 0.05 * np.array([0.48, -0.6, 0.64])]))
POSE = synth.look_at_pose(3).numpy()
ROOM = (0.8, 0.6, 1.0)       # a room small enough for 2 000 discs of the largest radius (5 cm) to cover its walls


def render_pair_scene():
    """-> (map, deformed map, settings at POSE, settings at DELTA POSE): 2 000 surface Gaussians without higher SH bands; the
    deformed map is the DEFINITION's (the kernel equals it bit for bit), its normals the activation's rule on the new rotations."""
    g = synth.surface_gaussians(2000, CAM, seed=11, half=ROOM)
    g = {k: v.clone() for k, v in g.items()}
    g["shs"][:, 1:] = 0
    raw8 = np.zeros((2000, 8), dtype=F32)
    raw8[:, 4:8] = g["rotations"].numpy()
    tick = np.random.default_rng(2).integers(0, 6, size=2000)
    table = lc.deform_table(np.broadcast_to(DELTA, (6, 4, 4)))
    x1, r1 = mdr.deform(g["xyz"].numpy(), raw8, tick, table)
    d = dict(g)
    d["xyz"] = torch.from_numpy(x1)
    q = torch.from_numpy(r1[:, 4:8])
    d["rotations"] = q / q.norm(dim=1, keepdim=True)
    d["normal"] = synth.normal_from_scale_rot(g["scales"], d["rotations"])
    from oracle import raster_oracle as ro
    sets = [ro.make_settings(CAM.H, CAM.W, CAM.fx, CAM.fy, CAM.cx, CAM.cy,
                             viewmatrix=torch.from_numpy(np.linalg.inv(P)).float().t().contiguous()) for P in (POSE, DELTA @ POSE)]
    return g, d, sets[0], sets[1], tick, table


def differing_pixels(out_a, normal_a, out_b, normal_b):
    """Pixels whose colour, depth or normal differ by more than 1e-4 between the render of the map (its normals turned by DELTA's
    rotation into the deformed world) and the render of the deformed map."""
    R = torch.from_numpy(DELTA[:3, :3]).float()

    def normal_map(out, normal):
        idx = out[3].reshape(-1).long()
        n = torch.zeros(idx.numel(), 3)
        n[idx >= 0] = normal[idx[idx >= 0]]
        return n
    na, nb = normal_map(out_a, normal_a) @ R.t(), normal_map(out_b, normal_b)
    H, W = out_a[0].shape[-2:]
    bad = ((out_a[0] - out_b[0]).abs() > 1e-4).any(0) | ((out_a[1] - out_b[1]).abs() > 1e-4).any(0)
    bad |= ((na - nb).abs() > 1e-4).any(1).reshape(H, W)
    return int(bad.sum()), float((out_a[6] < 0.5).float().mean())


def oracle_count():
    g, d, s0, s1, _, _ = render_pair_scene()
    out_a, _, _ = ru.oracle_run(s0, g)
    out_b, _, _ = ru.oracle_run(s1, d)
    return differing_pixels(out_a, g["normal"], out_b, d["normal"])


def test_render_equivalence():
    """The map rendered at POSE and the deformed map rendered at DELTA POSE (3 degrees, 5 cm, every tick) show the same picture:
    colour, depth and - turned with DELTA - normal.  The float32 rows moved by a float32 matrix and the float32 view matrix of
    the product pose are not the same numbers, so a few pixels flip one of the blend's discontinuous decisions; the CPU oracle
    (oracle/raster_oracle.py, float32), rendering the same pair, sets the scale: 0 of its 19 200 pixels differ by more
    than 1e-4 (95 % of the picture covered; computed on the CPU by this file's oracle_count(), which the test runs again).  The HIP renders may differ in as many, plus
    the 4 pixels the parity tests allow a map."""
    from rtg_slam_amd import _lib
    g, d, s0, s1, tick, table = render_pair_scene()
    got_x, got_r = run_kernel(g["xyz"].numpy(), np.concatenate([np.zeros((2000, 4), F32), g["rotations"].numpy()], 1),
                              tick.astype(np.int32), table)
    assert np.array_equal(bits(got_x), bits(d["xyz"].numpy()))                    # the kernel's rows ARE the rendered ones
    q = torch.from_numpy(got_r[:, 4:8])
    assert torch.equal(q / q.norm(dim=1, keepdim=True), d["rotations"])
    out_a, _ = ru.hip_run(s0, g)
    out_b, _ = ru.hip_run(s1, d)
    count, covered = differing_pixels(out_a, g["normal"], out_b, d["normal"])
    ref, _ = oracle_count()
    print(f"render equivalence: {count} of {CAM.H * CAM.W} pixels differ by more than 1e-4 on the device, {ref} in the oracle; "
          f"{100 * covered:.1f} % of the picture is covered")
    assert covered > 0.5
    assert count <= ref + 4


# ---- the map object ----

def test_deform_rows_moves_the_map_and_invalidates_what_was_derived():
    from rtg_slam_amd import map_optim as mo
    g = synth.surface_gaussians(3000, CAM, seed=4)
    packed = mo.pack_from_activated({k: v.to(DEV) for k, v in g.items()})
    opt = mo.ShardedMapOptimizer(packed, n_frozen=1000, capacity=4096)
    tick = opt.add_aux("add_tick", 1, torch.int32, 0)
    tick[:3000, 0] = torch.arange(3000, dtype=torch.int32, device=DEV) % 7
    before = opt.params.cpu().numpy()
    gd = opt.gaussian_data()
    normal_before = gd["normal"].clone()
    version, key = opt.version, opt.frozen_key
    D = np.stack([np.eye(4)] + [DELTA] * 6)
    table = torch.from_numpy(lc.deform_table(D)).to(DEV)
    opt.deform_rows(table)
    assert opt.version > version and opt.frozen_key != key and not opt._act_valid
    after = opt.params.cpu().numpy()
    t = (np.arange(3000) % 7).astype(np.int32)
    want_x, want_r = mdr.deform(before[:, :3], before[:, 51:59], t, table.cpu().numpy())
    assert np.array_equal(bits(after[:, :3]), bits(want_x)) and np.array_equal(bits(after[:, 51:59]), bits(want_r))
    assert np.array_equal(bits(after[:, 3:51]), bits(before[:, 3:51]))            # SH untouched
    assert np.array_equal(bits(after[t == 0]), bits(before[t == 0]))              # frozen and trainable rows alike
    moved = torch.from_numpy(t != 0).to(DEV)
    n1 = opt.gaussian_data()["normal"]
    R = torch.from_numpy(DELTA[:3, :3]).float().to(DEV)
    assert float((n1[moved] - normal_before[moved] @ R.t()).abs().max()) < 1e-5    # the activated copies were refreshed
    assert torch.equal(n1[~moved], normal_before[~moved])
    # a 64-bit tick array, and the refusals
    opt.deform_rows(torch.from_numpy(lc.deform_table(np.stack([np.eye(4)] + [pg.inverse(DELTA)] * 6))).to(DEV),
                    tick=tick[:, 0].long().contiguous())
    back = opt.params.cpu().numpy()
    assert np.abs(back[:, :3] - before[:, :3]).max() < 1e-5
    with pytest.raises(ValueError):
        opt.deform_rows(table.cpu())
    with pytest.raises(ValueError):
        opt.deform_rows(table, tick=tick[:100])
    with pytest.raises(ValueError):
        opt.deform_rows(table.double())
    opt.begin_global_optimization()
    with pytest.raises(RuntimeError):
        opt.deform_rows(table)
    opt.end_global_optimization()


def test_a_same_view_step_after_a_deformation_culls_the_whole_map():
    """The kept cull of the one-call map step (tests/test_cull_cache_gpu.py): steps on one view hit it; after deform_rows the next
    step must cull the whole map again, and with the cache's self-check on - every hit is compared with a full cull on the
    device - no mismatch is ever seen."""
    from rtg_slam_amd import map_optim as mo
    from rtg_slam_amd import rasterizer as rz
    from tests import test_cull_cache_gpu as cc
    ctx = rz.current_context()
    g = cc._scene(2)
    ctx.set_cull_cache(True)
    ctx.set_cull_cache_check(True)
    try:
        start = ctx.cull_cache_stats()
        packed = mo.pack_from_activated({k: v.to(DEV) for k, v in g.items()})
        opt = mo.ShardedMapOptimizer(packed, lr_col=mo.default_lr_columns() * 1e-4, capacity=cc.N + 4096)
        opt.add_aux("add_tick", 1, torch.int32, 0)
        settings = cc._settings(cc.MID, 1)
        gt_c, gt_d = cc._gt(cc.MID)
        table = torch.from_numpy(lc.deform_table(DELTA[None])).to(DEV)
        opt.begin_local_optimization()
        seen = []
        for k in range(12):
            if k == 7:
                opt.deform_rows(table)
            opt.step_slam(settings, gt_c, gt_d, None)
            st = ctx.cull_cache_stats()
            seen.append({n: st[n] - start[n] for n in ("hits", "full", "check_mismatches")})
        print("cull cache per step (deformation before step 7):", seen)
        assert seen[6]["hits"] >= 3                                              # the steps before hit ...
        assert seen[7]["hits"] == seen[6]["hits"] and seen[7]["full"] > seen[6]["full"]     # ... the step after it does not
        assert seen[11]["hits"] > seen[7]["hits"]                                # and the cache comes back
        assert seen[11]["check_mismatches"] == 0
    finally:
        ctx.set_cull_cache(True)
        ctx.set_cull_cache_check(False)
