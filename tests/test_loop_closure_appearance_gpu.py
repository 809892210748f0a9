"""loop_closure_candidates "appearance" end to end: the turn of tests/test_place_cpu.py (42 frames, the last six a revisit of the
first, offset by 54 mm and 3 degrees) mapped along a trajectory that drifted by 12 x UNIT a frame - 18 mm and 0.36 degrees, 749
mm at the last frame, beyond loop_closure_max_trans - so that the estimated poses show no loop at all.  Mode "pose" finds
nothing and changes nothing; mode "appearance" finds the revisits from the keyframes' thumbnails, registers them from the
shift's yaw alone and closes the loop.  And the choice switched off, or given as "pose", changes nothing at all.

The drift is the issue's 12 x UNIT: the keyframes stay [0, 2, 5, ..., 41] under it (asserted below)."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import pose_graph as pg
from tests.test_loop_closure_gpu import CAM, DEV, UNIT, drifted_poses, kf_rms, loop_args, straight_stream
from tests.test_place_cpu import DRIFT_SCALE, KEYFRAMES, turn_frames

pytestmark = pytest.mark.gpu

# what the closure's report held before there was a choice of candidates
REPORT_KEYS = {"keyframes", "frames", "options", "exposure_unknowns", "candidates", "edges", "changed", "seconds", "ate_rmse_m_before",
               "ate_rmse_m", "ate_rmse_aligned_m_before", "ate_rmse_aligned_m"}
OPTION_KEYS = {"min_gap", "max_trans", "max_rot_deg", "max_per_keyframe", "min_inlier_ratio", "max_rms", "max_correction_trans",
               "max_correction_rot_deg", "odometry_weights", "loop_weights", "huber"}
CANDIDATE_KEYS = {"accepted", "reason", "refine_reason", "iterations", "rank_min", "rms_geometric_before", "rms_geometric_after",
                  "device_s", "inliers", "valid_source_pixels", "inlier_ratio", "correction_trans", "correction_rot_deg", "a", "b",
                  "frame_a", "frame_b", "distance_m", "angle_deg"}


def test_a_loop_the_poses_do_not_show_is_closed_by_appearance():
    """Measured on an MI355X: the three candidates are the three revisits, (0, 12), (1, 13) and (2, 14), at scores 0.9915, 0.9980,
    0.9987, shifts +4, -1, -1 and depth_rel 0.0546, 0.0172, 0.0158 - the numpy definition's figures - while their estimated poses
    lie 640 - 706 mm and 7.6 - 15.5 degrees apart.  All three are accepted (inlier ratios 0.819, 0.944, 0.955; rms 0.27 - 0.36
    mm; corrections from the appearance guess 0.2 mm / 1.31 degrees, 53.8 mm / 0.14 degrees, 53.9 mm / 0.14 degrees) with Z
    0.19, 0.19 and 0.03 mm from the true relative pose (bound 5 mm).  The keyframes' rms translation error against the true
    poses falls from 435.62 to 24.33 mm, the ATE of all frames from 435.35 to 23.87 mm (bounds: half).  The first closure's
    largest correction is 707.70 mm, the second's 0.014 mm (bound: a tenth, 70.8 mm).  Describing the 15 keyframes takes 0.6
    ms, scoring the 15 pairs 0.2 ms, the whole closure 35 ms, 26 of them in the graph."""
    from rtg_slam_amd import slam
    fr = turn_frames()
    truth = [f[2] for f in fr]
    drifted = drifted_poses(truth, DRIFT_SCALE * UNIT)
    args = loop_args()
    torch.manual_seed(1)
    stream = ((d.to(DEV), c.to(DEV), drifted[k]) for k, (d, c, _) in enumerate(fr))
    mapper, tracker, rep = slam.run_sequence(CAM, stream, args, DEV, capacity=200_000)
    ids = list(mapper.keyframe_ids)
    assert ids == KEYFRAMES, ids
    M = len(ids)
    truth_kf = [truth[i] for i in ids]

    # mode "pose": the estimated poses show no loop
    poses_before = np.stack(tracker.pose_es)
    params_before = mapper.opt.params[:mapper.opt.N].clone()
    version = mapper.opt.version
    out = lc.LoopCloser(loop_args()).close(mapper, tracker)
    assert out["candidates"] == [] and out["edges"] == 0 and out["changed"] is False and "appearance" not in out
    assert set(out) == REPORT_KEYS
    assert np.array_equal(np.stack(tracker.pose_es), poses_before) and mapper.opt.version == version
    assert torch.equal(mapper.opt.params[:mapper.opt.N], params_before)

    # mode "appearance"
    rms_before = kf_rms([tracker.pose_es[i] for i in ids], truth_kf)
    ate_before = slam.ate_rmse(tracker.pose_es, truth)
    normals_before = [km["normal_map_w"].clone() for km in mapper.keymap_list]
    closer = lc.LoopCloser(loop_args(loop_closure_candidates="appearance"))
    out = closer.close(mapper, tracker)
    print("appearance:", out["appearance"], {k: round(v, 4) for k, v in out["seconds"].items()})
    print("candidates:", [(c["a"], c["b"], c["source"], round(c["score"], 4), c["shift"], round(c["depth_rel"], 4), c["reason"],
                           round(c["inlier_ratio"], 3), round(1e3 * c["rms_geometric_after"], 2), round(1e3 * c["correction_trans"], 1),
                           round(c["correction_rot_deg"], 2), round(c["distance_m"], 3), round(c["angle_deg"], 1))
                          for c in out["candidates"]])
    assert all(c["source"] == "appearance" for c in out["candidates"]) and out["appearance"]["thumbnail"] == [40, 30]
    assert out["appearance"]["candidates"] == len(out["candidates"]) and out["appearance"]["pairs_scored"] == 15
    accepted = [c for c in out["candidates"] if c["accepted"]]
    assert any(c["a"] < 3 and c["b"] >= M - 3 for c in accepted), out["candidates"]
    assert out["changed"] and out["edges"] == len(accepted) and mapper.opt.version > version
    for c in accepted:
        want = pg.inverse(truth_kf[c["a"]]) @ truth_kf[c["b"]]
        err = float(np.linalg.norm(np.asarray(c["Z"])[:3, 3] - want[:3, 3]))
        print(f"edge ({c['a']}, {c['b']}): Z {1e3 * err:.2f} mm from the true relative pose")
        assert err < 5e-3, (c["a"], c["b"], err)
    rms_after = kf_rms([tracker.pose_es[i] for i in ids], truth_kf)
    ate_after = slam.ate_rmse(tracker.pose_es, truth)
    print(f"keyframe rms translation error {1e3 * rms_before:.2f} -> {1e3 * rms_after:.2f} mm; ATE against the true poses "
          f"{1e3 * ate_before:.2f} -> {1e3 * ate_after:.2f} mm; largest correction {1e3 * out['correction_max_m']:.2f} mm")
    assert rms_after < 0.5 * rms_before
    assert ate_after < 0.5 * ate_before
    # the keyframes' frames and kept normals moved with the poses; frame 0 is held
    for k, kf in enumerate(mapper.keyframe_list):
        assert np.array_equal(kf.c2w.numpy(), tracker.pose_es[ids[k]])
    assert np.array_equal(tracker.pose_es[0], drifted[0])
    assert torch.equal(mapper.keymap_list[0]["normal_map_w"], normals_before[0])
    assert not torch.equal(mapper.keymap_list[-1]["normal_map_w"], normals_before[-1])
    # a second closure finds the same places and little left to correct
    again = closer.close(mapper, tracker)
    print(f"second closure: {again['edges']} edges, largest correction {1e3 * again.get('correction_max_m', 0.0):.3f} mm "
          f"against {1e3 * out['correction_max_m']:.3f} mm")
    assert again["edges"] >= 1 and again["correction_max_m"] < 0.1 * out["correction_max_m"]


def test_off_means_off(monkeypatch):
    """The straight stream of tests/test_loop_closure_gpu.py at loop_closure_min_gap 1, so that there ARE pose candidates: with
    the key absent and with "pose" the report holds the keys it held before, no candidate carries `source`, and neither place
    kernel is launched.  gaussian_update_iter = 0 makes two runs of the same arguments bit-reproducible."""
    from rtg_slam_amd import _lib, slam
    lib = _lib.load()
    calls = {"rtgs_place_describe": 0, "rtgs_place_scores": 0}
    for name in calls:
        def counted(*a, _real=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    runs = {}
    for name, over in (("absent", {}), ("pose", {"loop_closure_candidates": "pose"}), ("both", {"loop_closure_candidates": "both"})):
        args = loop_args(gaussian_update_iter=0, keyframe_trans_thes=0.01, loop_closure=True, loop_closure_min_gap=1, **over)
        torch.manual_seed(1)
        before = dict(calls)
        runs[name] = slam.run_sequence(CAM, straight_stream(), args, DEV, capacity=100_000, final_global=False)
        if name != "both":
            assert calls == before == {"rtgs_place_describe": 0, "rtgs_place_scores": 0}
    assert not hasattr(loop_args(), "loop_closure_candidates")
    reps = {k: v[2]["loop_closure"] for k, v in runs.items()}
    for name in ("absent", "pose"):
        rep = reps[name]
        assert len(rep["candidates"]) >= 1
        assert set(rep) - {"graph", "correction_max_m", "correction_mean_m", "correction_max_deg"} == REPORT_KEYS
        assert set(rep["options"]) == OPTION_KEYS and set(rep["seconds"]) - {"graph", "apply"} == {"candidates", "registration", "total"}
        assert all(set(c) == CANDIDATE_KEYS for c in rep["candidates"])
    strip = lambda c: {k: v for k, v in c.items() if k != "device_s"}
    assert [strip(c) for c in reps["absent"]["candidates"]] == [strip(c) for c in reps["pose"]["candidates"]]
    assert np.array_equal(np.stack(runs["absent"][1].pose_es), np.stack(runs["pose"][1].pose_es))
    assert torch.equal(runs["absent"][0].opt.params[:runs["absent"][0].opt.N], runs["pose"][0].opt.params[:runs["pose"][0].opt.N])
    # "both": the pose candidates first, exactly as before, then what appearance adds; the kernels did run
    both = reps["both"]
    n_kf = both["keyframes"]
    assert calls == {"rtgs_place_describe": n_kf, "rtgs_place_scores": 1}
    pose_part = [c for c in both["candidates"] if c["source"] == "pose"]
    assert both["candidates"][:len(pose_part)] == pose_part
    assert [(c["a"], c["b"]) for c in pose_part] == [(c["a"], c["b"]) for c in reps["absent"]["candidates"]]
    assert all(c["source"] == "appearance" and {"score", "shift", "depth_rel"} <= set(c) for c in both["candidates"][len(pose_part):])
    assert len({(c["a"], c["b"]) for c in both["candidates"]}) == len(both["candidates"])
    assert both["appearance"]["mode"] == "both" and {"describe", "scores"} <= set(both["seconds"])
    print("both:", both["appearance"], [(c["a"], c["b"], c["source"], c["accepted"]) for c in both["candidates"]])


@pytest.mark.parametrize("over", [dict(loop_closure_candidates="x"), dict(loop_closure_thumb_width=0),
                                  dict(loop_closure_thumb_width=8, loop_closure_max_shift=4), dict(loop_closure_max_shift=20),
                                  dict(loop_closure_max_shift=-1), dict(loop_closure_min_score=1.5), dict(loop_closure_min_score=-1.5),
                                  dict(loop_closure_max_depth_rel=-0.1)])
def test_invalid_values(over):
    with pytest.raises(ValueError):
        lc.LoopCloser(loop_args(**over))
    lc.LoopCloser(loop_args(loop_closure_candidates="both", loop_closure_thumb_width=8, loop_closure_max_shift=3,
                            loop_closure_min_score=-1.0, loop_closure_max_depth_rel=0.0))
