"""The host side of the loop closure without a device: loop_closure.find_candidates / frame_corrections / deform_table, and the
definition of rtgs_map_deform (tests/map_deform_reference.py) against exact arithmetic and the package's quaternion convention."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import pose_graph as pg
from rtg_slam_amd import synth
from rtg_slam_amd.rgbd_align import se3_exp, se3_log
from tests import map_deform_reference as mdr

F32 = np.float32
DELTA_A = se3_exp([0.01, -0.03, 0.02, 0.04, -0.01, 0.02])
DELTA_B = se3_exp([-0.02, 0.05, 0.01, -0.03, 0.05, 0.01])


def rows(n, seed=0):
    """-> (xyz [n,3], raw8 [n,8]) float32 of a plausible map: metres, raw quaternions of norm 0.5 .. 2."""
    rng = np.random.default_rng(seed)
    xyz = (rng.normal(size=(n, 3)) * 2.0).astype(F32)
    raw8 = rng.normal(size=(n, 8)).astype(F32)
    q = raw8[:, 4:8]
    raw8[:, 4:8] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n, 1))
    return xyz, raw8.astype(F32)


def test_fmaf_is_correctly_rounded():
    rng = np.random.default_rng(11)
    a, b = rng.normal(size=400).astype(F32), rng.normal(size=400).astype(F32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.normal(size=400) * 1e-7)).astype(F32)       # heavy cancellation
    c[::3] = rng.normal(size=c[::3].shape).astype(F32)
    # halfway cases of the double rounding: a b + c lies a hair beside the middle of two float32
    a[:4], b[:4] = F32(1 + 2.0 ** -12), F32(1 + 2.0 ** -12)
    c[:4] = [F32(2.0 ** -30), F32(-2.0 ** -30), F32(2.0 ** -60), F32(-2.0 ** -60)]
    got = mdr.fmaf(a, b, c)
    for k in range(a.size):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        lo = F32(float(exact))                          # float(Fraction) rounds correctly to double; then find the nearest float32
        cands = [np.nextafter(lo, F32(-np.inf)), lo, np.nextafter(lo, F32(np.inf))]
        dist = [abs(Fraction(float(x)) - exact) for x in cands]
        best = min(dist)
        winners = [x for x, d in zip(cands, dist) if d == best]
        if len(winners) == 2:                           # an exact tie: to even
            winners = [x for x in winners if (np.array(x).view(np.int32) & 1) == 0]
        assert got[k] == winners[0], (k, a[k], b[k], c[k], got[k], winners)


def test_frame_corrections_hand_made():
    ids = [0, 4, 10]
    old = [np.eye(4), se3_exp([0, 0.1, 0, 0.2, 0, 0]), se3_exp([0, 0.3, 0, 0.5, 0, 0.1])]
    new = [old[0], DELTA_A @ old[1], DELTA_B @ old[2]]
    D = lc.frame_corrections(ids, old, new, 14)
    assert D.shape == (14, 4, 4) and D.dtype == np.float64
    assert np.array_equal(D[0], np.eye(4))                                        # on an unchanged keyframe: the identity itself
    assert np.abs(D[4] - DELTA_A).max() < 1e-15 and np.abs(D[10] - DELTA_B).max() < 1e-15
    assert np.abs(se3_log(D[2]) - 0.5 * se3_log(DELTA_A)).max() < 1e-14            # halfway from the identity
    mid = DELTA_A @ se3_exp(0.5 * se3_log(pg.inverse(DELTA_A) @ DELTA_B))          # halfway between two keyframes
    assert np.abs(D[7] - mid).max() < 1e-14
    assert np.abs(se3_log(pg.inverse(D[4]) @ D[7]) - se3_log(pg.inverse(D[7]) @ D[10])).max() < 1e-13
    for f in (11, 12, 13):                                                         # after the last keyframe
        assert np.array_equal(D[f], D[10])
    for f in range(14):
        assert np.abs(D[f][:3, :3] @ D[f][:3, :3].T - np.eye(3)).max() < 1e-14 and np.array_equal(D[f][3], [0, 0, 0, 1])
    same = lc.frame_corrections(ids, old, old, 14)                                 # identity in, identity out - exactly
    assert np.array_equal(same, np.broadcast_to(np.eye(4), (14, 4, 4)))
    assert np.array_equal(lc.deform_table(same), np.broadcast_to(mdr.IDENTITY_ROW, (14, 16)))
    for bad in (([1, 4], old[:2], new[:2], 14), ([0, 4, 4], old, new, 14), (ids, old, new, 10), (ids, old[:2], new, 14)):
        with pytest.raises(ValueError):
            lc.frame_corrections(*bad)


def test_definition_composed_with_its_inverse_restores_the_rows():
    xyz, raw8 = rows(4000, seed=3)
    tick = np.random.default_rng(4).integers(-3, 9, size=4000)
    D = np.stack([np.eye(4), DELTA_A, DELTA_B, DELTA_A @ DELTA_B, pg.inverse(DELTA_B), DELTA_A])
    fwd, back = lc.deform_table(D), lc.deform_table(np.stack([pg.inverse(d) for d in D]))
    x1, r1 = mdr.deform(xyz, raw8, tick, fwd)
    x2, r2 = mdr.deform(x1, r1, tick, back)
    moved = np.clip(tick, 0, 5) != 0
    assert np.array_equal(x1[~moved].view(np.int32), xyz[~moved].view(np.int32))
    assert np.abs(x1[moved] - xyz[moved]).max() > 0.01
    # a few ulps of the largest coordinate involved (the rotation mixes the axes) and of the quaternion's norm
    scale = np.maximum(np.abs(xyz).max(axis=1, keepdims=True), np.abs(x1).max(axis=1, keepdims=True))
    assert (np.abs(x2 - xyz) <= 8 * np.spacing(scale.astype(F32))).all()
    qn = np.linalg.norm(raw8[:, 4:8], axis=1, keepdims=True)
    assert (np.abs(r2[:, 4:8] - raw8[:, 4:8]) <= 8 * np.spacing(qn.astype(F32))).all()
    assert np.array_equal(r2[:, :4].view(np.int32), raw8[:, :4].view(np.int32))    # opacity and scales are not touched
    assert np.abs(np.linalg.norm(r1[:, 4:8], axis=1, keepdims=True) / qn - 1).max() < 1e-6       # the raw norm is kept


def test_quaternion_convention():
    """R(q') = R_D R(q) in the package's convention (synth.quat_to_rotmat, on the normalised quaternion)."""
    xyz, raw8 = rows(500, seed=5)
    table = lc.deform_table(np.stack([DELTA_A, DELTA_B]))
    tick = np.arange(500) % 2
    _, r1 = mdr.deform(xyz, raw8, tick, table)
    unit = lambda q: q / np.linalg.norm(q, axis=1, keepdims=True)
    R0 = synth.quat_to_rotmat(torch.from_numpy(unit(raw8[:, 4:8].astype(np.float64)))).reshape(-1, 3, 3).numpy()
    R1 = synth.quat_to_rotmat(torch.from_numpy(unit(r1[:, 4:8].astype(np.float64)))).reshape(-1, 3, 3).numpy()
    RD = np.stack([DELTA_A[:3, :3], DELTA_B[:3, :3]])[tick]
    assert np.abs(R1 - RD @ R0).max() < 1e-6
    for D in (DELTA_A, DELTA_B, se3_exp([0, 3.1, 0, 0, 0, 0]), se3_exp([2.0, -2.0, 1.0, 0, 0, 0]), np.eye(4)):
        q = lc.rotmat_to_quat(D[:3, :3])
        assert abs(np.dot(q, q) - 1) < 1e-15 and q[0] >= 0
        assert np.abs(synth.quat_to_rotmat(torch.from_numpy(q[None])).reshape(3, 3).numpy() - D[:3, :3]).max() < 1e-14


def test_find_candidates_hand_made():
    """Twelve keyframes along x, 10 cm apart, then four that come back next to keyframes 0 .. 3, the last one turned away."""
    poses = [se3_exp([0, 0, 0, 0.1 * k, 0, 0]) for k in range(12)]
    back = [se3_exp([0, 0, 0, 0.1 * k + 0.02, 0.01, 0]) for k in (3, 2, 1)] + [se3_exp([0, np.deg2rad(40), 0, 0.0, 0.01, 0])]
    poses += back
    ids = list(range(0, 3 * len(poses), 3))
    got = lc.find_candidates(poses, ids, min_gap=9, max_trans=0.15, max_rot_deg=30, max_per_keyframe=2)
    pairs = [(a, b) for a, b, _, _ in got]
    # keyframe 12 sits at x = 0.32: nearest 3 (2.2 cm), then 4 (8.1 cm) - but 12 - 4 = 8 < 9 is too recent -, then 2 (12 cm)
    assert pairs == [(3, 12), (2, 12), (2, 13), (3, 13), (1, 14), (2, 14)], pairs
    assert all(b - a >= 9 for a, b in pairs)
    d = {(a, b): (dist, ang) for a, b, dist, ang in got}
    assert abs(d[(3, 12)][0] - np.hypot(0.02, 0.01)) < 1e-12 and d[(3, 12)][1] < 1e-6
    one = lc.find_candidates(poses, ids, 9, 0.15, 30, 1)
    assert [(a, b) for a, b, _, _ in one] == [(3, 12), (2, 13), (1, 14)]
    wide = lc.find_candidates(poses, ids, 9, 0.15, 45, 2)                          # keyframe 15 turned 40 degrees: found only now
    assert [(a, b) for a, b, _, _ in wide][-2:] == [(0, 15), (1, 15)]
    assert lc.find_candidates(poses[:10], ids[:10], 10, 10.0, 180, 2) == []          # too short for the gap
    assert lc.find_candidates(poses, ids, 9, 0.15, 30, 2) == got
    assert [(a, b) for a, b, _, _ in lc.find_candidates(poses, ids, 10, 0.15, 30, 2)][0] == (2, 12)      # 12 - 3 = 9 is then too recent                   # deterministic
    with pytest.raises(ValueError):
        lc.find_candidates(poses, ids[:-1], 10, 0.15, 30, 2)
    with pytest.raises(ValueError):
        lc.find_candidates(poses, ids, 0, 0.15, 30, 2)


def test_loop_closer_reads_its_options():
    from types import SimpleNamespace
    c = lc.LoopCloser(SimpleNamespace(icp_downscales=[0.25, 0.5, 1.0], loop_closure_min_gap=5, loop_closure_loop_weights=[4, 9]))
    assert c.cfg.min_gap == 5 and c.cfg.max_trans == 0.5 and c.cfg.loop_weights == (4.0, 9.0) and not c.refiner.exposure
    assert lc.LoopCloser(SimpleNamespace(map_exposure=True)).refiner.exposure
    assert lc.LoopCloser(SimpleNamespace(rgbd_refine_exposure=True)).refiner.exposure
    for bad in (dict(loop_closure_min_gap=0), dict(loop_closure_max_trans=-1.0), dict(loop_closure_min_inlier_ratio=1.5),
                dict(loop_closure_loop_weights=[1.0]), dict(loop_closure_odometry_weights=[0.0, 0.0]), dict(loop_closure_huber=0.0)):
        with pytest.raises(ValueError):
            lc.LoopCloser(SimpleNamespace(**bad))
