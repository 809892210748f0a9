"""The precondition of tests/test_relocalisation_gpu.py from the definitions alone (tests/place_reference.py,
tests/keypoint_reference.py, tests/rigid_ransac_reference.py and the CPU registration of tests/test_keypoints_cpu.py), and the
relocalise_* keys and flags.

THE RETURN FRAME of that stream - the view 3 degrees and (0.04, -0.02, 0.03) m beside the yaw-11 view - against the keyframe
views of part A (yaw 0, 2, 5, .., 29 at CENTRE), measured with the definitions at the defaults (S = 4, tw = 40):
    keyframe view   score    shift   depth_rel   matches   inliers
    yaw 11          0.9680    -2      0.0284        75        73
    yaw 14          0.9873     0      0.0124        85        81
    yaw 17          0.9826    +1      0.0174        81        75
From the keypoint pose against the yaw-14 view the registration is accepted (correction 4.05 mm) and lands 0.09 mm from the truth."""
import numpy as np
import pytest

from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import pose_graph as pg
from rtg_slam_amd import relocalisation as rl
from tests import keypoint_reference as ref
from tests import place_reference as pref
from tests import rigid_ransac_reference as rr
from tests.test_keypoints_cpu import K_CAM, RIGHT, features_of, textured_view, view_pose
from tests.test_loop_closure_gpu import CAM, loop_args
from tests.test_place_cpu import NumpyRefiner

F32 = np.float32
RETURN = view_pose(11.0 + RIGHT["54 mm / 3 deg"][0], RIGHT["54 mm / 3 deg"][1])


def thumbs(T):
    d, c = textured_view(T)
    return pref.describe(c.numpy(), d.numpy(), 40)


def pyramids(T):
    import torch
    from oracle import icp_oracle as io
    from tests import rgbd_align_reference as rar
    d, c = textured_view(T)
    vp = io.vertex_pyramid(d, torch.tensor(K_CAM, dtype=torch.float32), 3)
    return {"vertex": [x.numpy() for x in vp], "normal": [x.numpy() for x in io.normal_pyramid(vp)], "intensity": rar.intensity_pyramid(c.numpy(), 3)}


def test_the_return_frame_can_be_recovered_by_the_definitions():
    cfg = lc.LoopCloser(loop_args())
    B = thumbs(RETURN)
    fb = features_of(RETURN)
    best = None
    for yaw in (11.0, 14.0, 17.0):
        Ta = view_pose(yaw)
        A = thumbs(Ta)
        sc, sh, rel = pref.pair_scores(A[0][None], A[1][None], A[2][None], B[0][None], B[1][None], B[2][None], 4)
        fa = features_of(Ta)
        fit = rr.pair(ref.match(fb["desc"], fa["desc"]), ref.match(fa["desc"], fb["desc"]), fa["xyz"], fb["xyz"])
        print(f"yaw {yaw:g}: score {float(sc[0]):.4f}, shift {int(sh[0]):+d}, depth_rel {float(rel[0]):.4f}, {fit['n']} matches, {fit['inliers']} inliers")
        if float(sc[0]) >= cfg.place.min_score and float(rel[0]) <= cfg.place.max_depth_rel and (best is None or fit["inliers"] > best[1]["inliers"]):
            best = (Ta, fit)
    assert best is not None and best[1]["inliers"] >= cfg.keypoints.cfg.min_inliers == 8
    Ta, fit = best
    want = pg.inverse(Ta) @ RETURN
    r = lc.register_pair(NumpyRefiner(), pyramids(RETURN), pyramids(Ta), fit["T"], K_CAM.astype(F32), [0.25, 0.5, 1.0], cfg.cfg)
    err = float(np.linalg.norm(r["Z"][:3, 3] - want[:3, 3]))
    print(f"registration: {r['reason']}, {1e3 * err:.2f} mm from the truth, correction {1e3 * r['correction_trans']:.2f} mm")
    assert r["accepted"], r["reason"]
    assert err < 5e-3


def test_the_keys_default_to_the_loop_closures_and_are_validated():
    from rtg_slam_amd import keypoints as kp
    r = rl.Relocaliser(loop_args(use_gt_pose=False, relocalise=True))
    assert r.options() == dict(candidates=3, min_score=lc.DEFAULTS["loop_closure_min_score"], max_depth_rel=lc.DEFAULTS["loop_closure_max_depth_rel"],
                               thumb_width=40, max_shift=4, min_inliers=kp.DEFAULTS["min_inliers"], min_inlier_ratio=0.3, max_rms=0.02,
                               max_correction_trans=0.2, max_correction_rot_deg=5.0)
    r = rl.Relocaliser(loop_args(use_gt_pose=False, loop_closure_min_score=0.8, loop_closure_keypoint_min_inliers=12, relocalise_max_shift=3,
                                 relocalise_candidates=5, relocalise_max_rms=0.01))
    assert (r.place.min_score, r.kc.min_inliers, r.place.max_shift, r.candidates, r.cfg.max_rms) == (0.8, 12, 3, 5, 0.01)
    for over in (dict(relocalise_candidates=0), dict(relocalise_min_score=-1.5), dict(relocalise_max_depth_rel=-1.0), dict(relocalise_thumb_width=0),
                 dict(relocalise_max_shift=-1), dict(relocalise_max_shift=20), dict(relocalise_min_inliers=2), dict(relocalise_min_inlier_ratio=-0.1),
                 dict(relocalise_max_rms=-0.1), dict(relocalise_max_correction_trans=-1.0), dict(relocalise_max_correction_rot_deg=-1.0),
                 dict(use_gt_pose=True), dict(loop_closure_keypoint_ransac_iters=65536)):
        with pytest.raises(ValueError):
            rl.Relocaliser(loop_args(**dict(dict(use_gt_pose=False), **over)))
    with pytest.raises(ValueError, match="relocalise_min_inliers"):
        rl.Relocaliser(loop_args(use_gt_pose=False, relocalise_min_inliers=2))
    with pytest.raises(RuntimeError):
        rl.Relocaliser(loop_args(use_gt_pose=False), world=4)
    with pytest.raises(ValueError):
        rl.refuse_pipeline(loop_args(relocalise=True))
    rl.refuse_pipeline(loop_args())


def test_the_cli_flags_set_the_keys_only_when_given():
    from types import SimpleNamespace
    from rtg_slam_amd import __main__ as cli
    parse = lambda argv: cli.build_parser().parse_args(["slam", "--config", "x.yaml"] + argv)
    base = lambda: SimpleNamespace(**vars(loop_args(use_gt_pose=False)))
    args = base()
    before = dict(vars(args))
    assert cli._apply_relocalise(args, parse([])) is None and vars(args) == before
    assert cli._apply_relocalise(args, parse(["--relocalise", "--relocalise-candidates", "2", "--relocalise-min-score", "0.85",
                                              "--relocalise-min-inliers", "10"])) is None
    assert {k: v for k, v in vars(args).items() if k not in before} == dict(relocalise=True, relocalise_candidates=2, relocalise_min_score=0.85,
                                                                            relocalise_min_inliers=10)
    for name, *_ in cli.RELOCALISE_FLAGS:
        assert name == "candidates" or "relocalise_" + name in rl.KEYS
    assert set(rl.KEYS) == {"relocalise_" + name for name, *_ in cli.RELOCALISE_FLAGS} - {"relocalise_candidates"}
    said = cli._apply_relocalise(base(), parse(["--relocalise-candidates", "2"]))
    assert said is not None and "needs --relocalise" in said
    said = cli._apply_relocalise(base(), parse(["--relocalise", "--relocalise-candidates", "0"]))
    assert said is not None and "relocalise_candidates" in said
    said = cli._apply_relocalise(SimpleNamespace(**vars(loop_args())), parse(["--relocalise"]))
    assert said is not None and "use_gt_pose" in said
