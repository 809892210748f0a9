"""tests/rigid_ransac_reference.py, the definition of rtgs_rigid_ransac, on known cases, and against keypoints.ransac_rigid - the
host's RANSAC, which fits by LAPACK's SVD - on the pairs of tests/test_keypoints_cpu.py; then the new keys.

Measured (the definition against ransac_rigid, the same matches in):
    pair                           matches   inliers (both)   max |T - T_host|
    54 mm / 3 deg                     72          72             < 1e-13
    0.3 m / 10 deg                    42          34             < 1e-13
    0.5 m / 12 deg, 8 deg roll        36          23             < 1e-13
    wide (1, 13)                      59          49             < 1e-13
    wide (2, 14)                      49          40             < 1e-13
No case had a residual within 1e-9 m of inlier_dist: none is left out."""
import numpy as np
import pytest

from rtg_slam_amd import keypoints as kp
from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd.rgbd_align import se3_exp
from tests import keypoint_reference as ref
from tests import rigid_ransac_reference as rr
from tests.test_keypoints_cpu import RIGHT, WIDE_PAIRS, features_of, view_pose, wide_turn_frames
from tests.test_loop_closure_gpu import loop_args
from tests.test_place_cpu import KEYFRAMES

T_TRUE = se3_exp([0.1, -0.3, 0.05, 0.4, -0.2, 0.3])


def test_an_exact_pose_under_half_gross_outliers():
    rng = np.random.default_rng(7)
    pb = rng.uniform(-2, 2, size=(40, 3)) + (0, 0, 3)
    pa = pb @ T_TRUE[:3, :3].T + T_TRUE[:3, 3]
    bad = rng.permutation(40)[:20]
    pa[bad] += rng.uniform(0.5, 2.0, size=(20, 3)) * rng.choice([-1, 1], size=(20, 3))
    r = rr.ransac(pa, pb)
    assert r["inliers"] == 20 and not r["mask"][bad].any() and r["h"] >= 0 and r["rms"] < 1e-12
    assert np.abs(r["T"] - T_TRUE).max() < 1e-12 and np.array_equal(r["T"][3], [0, 0, 0, 1])
    again = rr.ransac(pa, pb)
    assert np.array_equal(again["T"], r["T"]) and again["rms"] == r["rms"] and again["h"] == r["h"]
    host = kp.ransac_rigid(pa, pb)
    assert np.array_equal(host[1], r["mask"]) and np.abs(host[0] - r["T"]).max() < 1e-12
    other = rr.ransac(pa, pb, seed=12345)                            # another stream of triplets, the same pose
    assert other["inliers"] == 20 and np.abs(other["T"] - T_TRUE).max() < 1e-12


def test_too_few_and_collinear_matches_give_no_result():
    p = np.array([[0, 0, 1.0], [1, 0, 1], [0, 1, 2]])
    for n in (0, 2):
        r = rr.ransac(p[:n], p[:n])
        assert r["h"] == -1 and r["inliers"] == 0 and not r["T"].any() and r["rms"] == 0.0 and r["mask"].shape == (n,)
    assert rr.ransac(p, p)["inliers"] == 3
    line = np.outer(np.linspace(0, 3, 12), [1.0, 0.5, 0.2]) + (0, 0, 2)
    assert rr.ransac(line[:3], line[:3])["h"] == -1 and rr.ransac(line, line)["h"] == -1
    near = line.copy()
    near[:, 1] += 1e-3 * np.sin(np.arange(12))                       # 1 mm off a 3.4 m line: below the rule's 5.74 degrees
    assert rr.ransac(near, near)["h"] == -1
    same = np.repeat(p[:1], 5, axis=0)                               # |e|^2 = 0 is not > 1e-18
    assert rr.ransac(same, same)["h"] == -1
    # the rule without norms is _spread's: |c| >= 0.1 |e1| |e2|
    rng = np.random.default_rng(3)
    tri = rng.normal(size=(200, 3, 3)) * np.array([1.0, 0.05, 0.05])
    assert np.array_equal(rr.spread(tri), [bool(kp._spread(t)) for t in tri]) and 20 < rr.spread(tri).sum() < 180
    with pytest.raises(ValueError):
        rr.ransac(p, p, iters=0)
    with pytest.raises(ValueError):
        rr.ransac(p, p, iters=65536)


def test_a_tie_in_the_count_goes_to_the_earlier_h():
    """Two rigid groups of six, 1 m apart in a: every valid triplet within one group counts six, mixed ones fewer; the winner is
    the first h whose triplet lies within one group, whichever group that is."""
    rng = np.random.default_rng(11)
    pb = rng.uniform(-1, 1, size=(12, 3)) + (0, 0, 3)
    pa = pb @ T_TRUE[:3, :3].T + T_TRUE[:3, 3]
    pa[6:] += (1.0, 0.0, 0.0)
    r = rr.ransac(pa, pb, iters=64)
    idx = rr.triplets(12, 64, 0)
    pure = [h for h in range(64) if len(set(idx[h].tolist())) == 3 and len({i // 6 for i in idx[h].tolist()}) == 1
            and rr.spread(pa[idx[h]]) and rr.spread(pb[idx[h]])]
    groups = {int(idx[h][0]) // 6 for h in pure}
    assert groups == {0, 1} and r["h"] == pure[0] and r["inliers"] == 6
    assert r["mask"].tolist() == [int(idx[pure[0]][0]) // 6 == k // 6 for k in range(12)]


def test_the_cap_on_the_matches():
    n = rr.CAP + 7
    m_ba = np.stack([np.arange(n), np.full(n, 10), np.full(n, 100)], axis=1).astype(np.int32)
    m_ba[5] = (-1, 257, 257)
    m_ab = np.stack([np.arange(n), np.full(n, 10), np.full(n, 100)], axis=1).astype(np.int32)
    ij, survivors = rr.filter_matches(m_ba, m_ab)
    assert survivors == n - 1 and len(ij) == rr.CAP == 1024 and ij[:6] == [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (6, 6)]
    assert ij[-1] == (rr.CAP, rr.CAP)                                # dropped in order: the first 1024 survivors stay
    assert [(i, j) for i, j, _ in kp.filter_matches(m_ba, m_ab)][:rr.CAP] == ij
    assert rr.filter_matches(m_ba[:, [0, 1, 2]], m_ab[:3])[1] == 3   # an index beyond a's table is not followed
    rng = np.random.default_rng(2)
    x = rng.uniform(-2, 2, size=(n, 3)) + (0, 0, 3)
    r = rr.pair(m_ba, m_ab, x @ T_TRUE[:3, :3].T + T_TRUE[:3, 3], x, iters=8)
    assert (r["n"], r["survivors"], r["inliers"]) == (rr.CAP, n - 1, rr.CAP) and r["ij"].shape == (rr.CAP, 2)
    with pytest.raises(ValueError):
        rr.ransac(x, x)


@pytest.mark.parametrize("axis", [(1.0, 0, 0), (0, 1.0, 0), (0, 0, 1.0), (0.6, 0.0, 0.8)])
def test_a_half_turn_where_w_is_zero(axis):
    u = np.asarray(axis)
    R = 2.0 * np.outer(u, u) - np.eye(3)                             # the rotation by 180 degrees about u: quaternion (0, u)
    rng = np.random.default_rng(5)
    pb = rng.uniform(-2, 2, size=(30, 3))
    pa = pb @ R.T + (0.1, 0.2, 0.3)
    r = rr.ransac(pa, pb, iters=16)
    assert r["inliers"] == 30 and np.abs(r["T"][:3, :3] - R).max() < 1e-12 and np.abs(r["T"][:3, 3] - (0.1, 0.2, 0.3)).max() < 1e-12
    Rf, tf = rr.fit(pa, pb)
    assert np.abs(Rf - R).max() < 1e-12 and np.abs(Rf @ Rf.T - np.eye(3)).max() < 1e-14 and np.linalg.det(Rf) > 0.999


def test_fit_is_a_proper_rotation_also_for_mirrored_points():
    rng = np.random.default_rng(9)
    pb = rng.uniform(-1, 1, size=(20, 3))
    pa = pb * (1, 1, -1)                                             # a reflection: the closed form still returns a rotation
    Rf, _ = rr.fit(pa, pb)
    assert np.linalg.det(Rf) > 0.999 and np.abs(Rf @ Rf.T - np.eye(3)).max() < 1e-14
    Rk, _ = kp.kabsch(pb, pa)
    assert np.abs(Rk - Rf).max() < 1e-9


def matched_points(fa, fb):
    m = ref.filter_matches(ref.match(fb["desc"], fa["desc"]), ref.match(fa["desc"], fb["desc"]))
    return m, fa["xyz"][[j for _, j, _ in m]], fb["xyz"][[i for i, _, _ in m]]


def textured_pairs():
    out = [(name, view_pose(0.0), view_pose(yaw, off, roll)) for name, (yaw, off, roll) in sorted(RIGHT.items())]
    fr = wide_turn_frames()
    return out + [(f"wide {a, b}", fr[KEYFRAMES[a]][2], fr[KEYFRAMES[b]][2]) for a, b in WIDE_PAIRS]


@pytest.mark.parametrize("k", range(5))
def test_the_definition_against_the_hosts_ransac_on_the_textured_pairs(k):
    name, Ta, Tb = textured_pairs()[k]
    fa, fb = features_of(Ta), features_of(Tb)
    m, pa, pb = matched_points(fa, fb)
    host = kp.ransac_rigid(pa, pb)
    mine = rr.pair(ref.match(fb["desc"], fa["desc"]), ref.match(fa["desc"], fb["desc"]), fa["xyz"], fb["xyz"])
    assert mine["ij"].tolist() == [[i, j] for i, j, _ in m] and mine["n"] == mine["survivors"] == len(m)      # the filter is filter_matches
    res = np.sqrt(rr.residual2(mine["T"][:3, :3], mine["T"][:3, 3], pa, pb))
    edge = float(np.abs(res - 0.05).min())
    print(f"{name}: {len(m)} matches, {mine['inliers']} / {int(host[1].sum())} inliers, max |T - T_host| {np.abs(mine['T'] - host[0]).max():.2e}, "
          f"rms {mine['rms']:.6f} / {host[2]:.6f}, the residual nearest to inlier_dist misses it by {edge:.2e} m")
    assert edge > 1e-9                                               # no case sits on the threshold: none is left out
    assert np.array_equal(mine["mask"], host[1]) and mine["inliers"] >= 8
    assert np.abs(mine["T"] - host[0]).max() <= 1e-9 and abs(mine["rms"] - host[2]) <= 1e-9


def test_the_new_key_defaults_to_host_and_is_validated():
    ok = dict(loop_closure_candidates="appearance", loop_closure_appearance_init="keypoints")
    assert lc.LoopCloser(loop_args()).keypoints.ransac == "host" and lc.LoopCloser(loop_args(**ok)).keypoints.ransac == "host"
    assert lc.LoopCloser(loop_args(**ok, loop_closure_keypoint_ransac="device")).keypoints.ransac == "device"
    assert lc.LoopCloser(loop_args(**ok, loop_closure_keypoint_ransac="host")).keypoints.ransac == "host"
    assert "loop_closure_keypoint_ransac" not in lc.DEFAULTS and "ransac" not in kp.DEFAULTS and not hasattr(loop_args(), "loop_closure_keypoint_ransac")
    assert "ransac" not in vars(lc.LoopCloser(loop_args(**ok)).keypoints.cfg)
    for over in (dict(ok, loop_closure_keypoint_ransac="gpu"), dict(loop_closure_keypoint_ransac="device"),
                 dict(ok, loop_closure_keypoint_ransac="device", loop_closure_keypoint_ransac_iters=65536)):
        with pytest.raises(ValueError):
            lc.LoopCloser(loop_args(**over))
    lc.LoopCloser(loop_args(**ok, loop_closure_keypoint_ransac="host", loop_closure_keypoint_ransac_iters=65536))


def test_the_cli_flag_sets_the_key_only_when_given():
    from types import SimpleNamespace
    from rtg_slam_amd import __main__ as cli
    parse = lambda argv: cli.build_parser().parse_args(["slam", "--config", "x.yaml"] + argv)
    base = ["--loop-closure", "--loop-closure-candidates", "appearance", "--loop-closure-appearance-init", "keypoints"]
    args = SimpleNamespace()
    assert cli._apply_loop_closure(args, parse(base)) is None and not hasattr(args, "loop_closure_keypoint_ransac")
    args = SimpleNamespace()
    assert cli._apply_loop_closure(args, parse(base + ["--loop-closure-keypoint-ransac", "device"])) is None
    assert vars(args) == dict(loop_closure=True, loop_closure_candidates="appearance", loop_closure_appearance_init="keypoints",
                              loop_closure_keypoint_ransac="device")
    assert not any(flag == "keypoint_ransac" for flag, *_ in cli.LOOP_CLOSURE_FLAGS)
    said = cli._apply_loop_closure(SimpleNamespace(), parse(["--loop-closure-keypoint-ransac", "device"]))
    assert said is not None and "needs --loop-closure" in said
    said = cli._apply_loop_closure(SimpleNamespace(), parse(["--loop-closure", "--loop-closure-keypoint-ransac", "device"]))
    assert said is not None and "loop_closure_appearance_init" in said
    with pytest.raises(SystemExit):
        parse(base + ["--loop-closure-keypoint-ransac", "cuda"])
