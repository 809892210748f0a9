"""loop_closure_appearance_init end to end.  THE WIDE TURN of tests/test_keypoints_cpu.py - the turn of tests/test_place_cpu.py in
the textured room, its revisit frames 304 mm, 6 degrees of yaw and 3 degrees of roll away from the first views - mapped along a
trajectory that drifted by 12 x UNIT a frame, as tests/test_loop_closure_appearance_gpu.py drifts it.  With the key absent the
wide revisits are found by their thumbnails and refused: the yaw guess has no translation, so the registration's correction is
the whole 304 mm.  With "keypoints" the guess is the pose from the matched keypoints, a few millimetres off, and they are
accepted.  And the key absent or "yaw" launches nothing and reports nothing new; "keypoints_strict" on the smooth room, where no
pixel is a corner, refuses every candidate unregistered, and "keypoints" falls back to the yaw guess there."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import pose_graph as pg
from tests.test_keypoints_cpu import WIDE_PAIRS, reference_pose, wide_turn_frames
from tests.test_loop_closure_appearance_gpu import CANDIDATE_KEYS, OPTION_KEYS, REPORT_KEYS
from tests.test_loop_closure_gpu import CAM, DEV, UNIT, drifted_poses, kf_rms, loop_args
from tests.test_place_cpu import DRIFT_SCALE, KEYFRAMES, turn_frames

pytestmark = pytest.mark.gpu

KERNELS = ("rtgs_keypoint_detect", "rtgs_keypoint_describe", "rtgs_keypoint_match")
APPEARANCE_KEYS = {"mode", "thumbnail", "max_shift", "min_score", "max_depth_rel", "pairs_scored", "candidates", "candidates_new"}
APPEARANCE_CANDIDATE_KEYS = CANDIDATE_KEYS | {"source", "Z", "score", "shift", "depth_rel"}
KEYPOINT_OPTIONS = {"keypoint_threshold", "keypoint_cell", "keypoint_oriented", "keypoint_max_hamming", "keypoint_ratio",
                    "keypoint_ransac_iters", "keypoint_inlier_dist", "keypoint_min_inliers"}


def mapped(frames):
    """The frames mapped along the drifted trajectory -> mapper, tracker, the true poses.  Few map iterations: the closure reads
    the keyframes' own colour and depth, not the map."""
    from rtg_slam_amd import slam
    truth = [f[2] for f in frames]
    drifted = drifted_poses(truth, DRIFT_SCALE * UNIT)
    torch.manual_seed(1)
    stream = ((d.to(DEV), c.to(DEV), drifted[k]) for k, (d, c, _) in enumerate(frames))
    mapper, tracker, _ = slam.run_sequence(CAM, stream, loop_args(gaussian_update_iter=3), DEV, capacity=200_000)
    assert list(mapper.keyframe_ids) == KEYFRAMES, list(mapper.keyframe_ids)
    return mapper, tracker, truth


def count_kernels(monkeypatch):
    from rtg_slam_amd import _lib
    lib = _lib.load()
    calls = {name: 0 for name in KERNELS}
    for name in calls:
        def counted(*a, _real=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    return calls


def state(mapper, tracker):
    return np.stack(tracker.pose_es).copy(), mapper.opt.params[:mapper.opt.N].clone(), mapper.opt.version


def brief(out):
    return [(c["a"], c["b"], c.get("init_source"), c["reason"], c.get("keypoints")) for c in out["candidates"]]


def test_the_yaw_guess_refuses_the_wide_revisits():
    """Measured on an MI355X: candidates (0, 12), (1, 13), (2, 14); (0, 12) - frame 35, which was not moved - is accepted, the two wide
    pairs are refused: correction 0.304 m / 6.08 degrees and 0.304 m / 6.10 degrees beyond 0.2 m / 5 degrees."""
    mapper, tracker, truth = mapped(wide_turn_frames())
    out = lc.LoopCloser(loop_args(loop_closure_candidates="appearance")).close(mapper, tracker)
    print("yaw:", brief(out))
    by_pair = {(c["a"], c["b"]): c for c in out["candidates"]}
    for pair in WIDE_PAIRS:
        assert pair in by_pair, sorted(by_pair)                   # found by their thumbnails ..
        c = by_pair[pair]
        assert not c["accepted"] and c["reason"].startswith("correction "), c["reason"]      # .. and refused for their correction
        assert c["correction_trans"] > 0.2
        assert set(c) == APPEARANCE_CANDIDATE_KEYS
    assert set(out["appearance"]) == APPEARANCE_KEYS and not any(k.startswith("keypoints") for k in out["seconds"])


def test_the_keypoint_pose_closes_the_wide_revisits(monkeypatch):
    """Measured on an MI355X: 6 keyframes described, one match launch; (0, 12), (1, 13), (2, 14) have 57 / 59 / 49 matches and 53 / 49 /
    40 inliers, the definition's figures, and all start from the keypoint pose; the wide pairs' guesses lie 2.9 and 6.4 mm from the
    truth, their corrections are 2.7 mm / 0.04 degrees and 5.9 mm / 0.24 degrees, their Z 0.89 and 0.51 mm from the true relative
    pose (bound 5 mm).  Keyframe rms translation error 427.94 -> 23.24 mm, ATE 427.52 -> 22.83 mm (bounds: half), three edges.
    Seconds: features 12.9 ms (the process's first launches), match 0.1 ms, RANSAC 77 ms, registration 5 ms, graph 29 ms."""
    from rtg_slam_amd import slam
    frames = wide_turn_frames()
    mapper, tracker, truth = mapped(frames)
    calls = count_kernels(monkeypatch)
    ids = KEYFRAMES
    truth_kf = [truth[i] for i in ids]
    rms_before = kf_rms([tracker.pose_es[i] for i in ids], truth_kf)
    ate_before = slam.ate_rmse(tracker.pose_es, truth)
    closer = lc.LoopCloser(loop_args(loop_closure_candidates="appearance", loop_closure_appearance_init="keypoints"))
    out = closer.close(mapper, tracker)
    print("keypoints:", brief(out), out["appearance"], {k: round(v, 4) for k, v in out["seconds"].items()})
    by_pair = {(c["a"], c["b"]): c for c in out["candidates"]}
    in_candidates = {k for pair in by_pair for k in pair}
    assert calls == {"rtgs_keypoint_detect": len(in_candidates), "rtgs_keypoint_describe": len(in_candidates), "rtgs_keypoint_match": 1}
    for pair in WIDE_PAIRS:
        c = by_pair[pair]
        want = pg.inverse(truth_kf[pair[0]]) @ truth_kf[pair[1]]
        err = float(np.linalg.norm(np.asarray(c["Z"])[:3, 3] - want[:3, 3]))
        off = float(np.linalg.norm(np.asarray(c["init"])[:3, 3] - want[:3, 3]))
        print(f"edge {pair}: {c['keypoints']}, guess {1e3 * off:.1f} mm off, correction {1e3 * c['correction_trans']:.1f} mm / "
              f"{c['correction_rot_deg']:.2f} degrees, Z {1e3 * err:.2f} mm from the true relative pose")
        assert c["accepted"], c["reason"]
        assert c["init_source"] == "keypoints" and err < 5e-3
        assert set(c) == APPEARANCE_CANDIDATE_KEYS | {"init_source", "init", "keypoints"}
        assert set(c["keypoints"]) == {"a", "b", "matches", "inliers", "rms_m"} and np.asarray(c["init"]).shape == (4, 4)
        n, inl, T, _ = reference_pose(frames[ids[pair[0]]][2], frames[ids[pair[1]]][2])    # the definition, on the CPU
        assert (c["keypoints"]["matches"], c["keypoints"]["inliers"]) == (n, inl) and np.array_equal(np.asarray(c["init"]), T)
    assert set(out["appearance"]) == APPEARANCE_KEYS | KEYPOINT_OPTIONS | {"init", "keypoint_inits"}
    assert out["appearance"]["init"] == "keypoints" and out["appearance"]["keypoint_inits"] >= len(WIDE_PAIRS)
    assert {"keypoints_describe", "keypoints_match", "keypoints_ransac"} <= set(out["seconds"])
    assert set(out["options"]) == OPTION_KEYS
    rms_after = kf_rms([tracker.pose_es[i] for i in ids], truth_kf)
    ate_after = slam.ate_rmse(tracker.pose_es, truth)
    print(f"keyframe rms translation error {1e3 * rms_before:.2f} -> {1e3 * rms_after:.2f} mm; ATE against the true poses "
          f"{1e3 * ate_before:.2f} -> {1e3 * ate_after:.2f} mm; {out['edges']} edges")
    assert out["changed"] and rms_after < 0.5 * rms_before and ate_after < 0.5 * ate_before


def textured_straight_stream(n=6):
    from rtg_slam_amd import synth
    for p in synth.trajectory(n, seed=21):
        d = synth.box_room_depth(CAM, p)
        yield d.to(DEV), synth.box_room_texture_color(CAM, p, d).to(DEV), p.numpy()


def test_off_means_off(monkeypatch):
    """The straight stream of tests/test_loop_closure_gpu.py, in the textured room, at loop_closure_min_gap 1 and candidates "both", so that there are
    pose and appearance candidates: with the key absent and with "yaw" no rtgs_keypoint_* entry point is called, the two reports
    are equal, and their key sets are the ones of tests/test_loop_closure_appearance_gpu.py.  With "keypoints" (and candidates
    "appearance", so that the pairs are not taken by the poses first) the kernels run: once per keyframe in a candidate, and one
    match launch."""
    from rtg_slam_amd import slam
    calls = count_kernels(monkeypatch)
    runs = {}
    for name, over in (("absent", {}), ("yaw", {"loop_closure_appearance_init": "yaw"}),
                       ("keypoints", {"loop_closure_appearance_init": "keypoints", "loop_closure_candidates": "appearance"})):
        args = loop_args(**dict(dict(gaussian_update_iter=0, keyframe_trans_thes=0.01, loop_closure=True, loop_closure_min_gap=1,
                                     loop_closure_candidates="both"), **over))
        torch.manual_seed(1)
        runs[name] = slam.run_sequence(CAM, textured_straight_stream(), args, DEV, capacity=100_000, final_global=False)
        if name != "keypoints":
            assert calls == {k: 0 for k in KERNELS}
    reps = {k: v[2]["loop_closure"] for k, v in runs.items()}
    extra = {"graph", "correction_max_m", "correction_mean_m", "correction_max_deg"}
    for name in ("absent", "yaw"):
        rep = reps[name]
        assert set(rep) - extra == REPORT_KEYS | {"appearance"} and set(rep["options"]) == OPTION_KEYS
        assert set(rep["appearance"]) == APPEARANCE_KEYS
        assert set(rep["seconds"]) - {"graph", "apply"} == {"candidates", "registration", "total", "describe", "scores"}
        assert len(rep["candidates"]) >= 1
        for c in rep["candidates"]:
            assert set(c) == (APPEARANCE_CANDIDATE_KEYS if c["source"] == "appearance" else CANDIDATE_KEYS | {"source", "Z"})
    strip = lambda c: {k: v for k, v in c.items() if k != "device_s"}
    assert [strip(c) for c in reps["absent"]["candidates"]] == [strip(c) for c in reps["yaw"]["candidates"]]
    assert np.array_equal(np.stack(runs["absent"][1].pose_es), np.stack(runs["yaw"][1].pose_es))
    assert torch.equal(runs["absent"][0].opt.params[:runs["absent"][0].opt.N], runs["yaw"][0].opt.params[:runs["yaw"][0].opt.N])
    on = reps["keypoints"]
    kfs = {k for c in on["candidates"] for k in (c["a"], c["b"])}
    print("keypoints on the straight stream:", brief(on), calls)
    assert len(on["candidates"]) >= 1 and all(c["source"] == "appearance" and c["keypoints"]["a"] > 0 for c in on["candidates"])
    assert calls == {"rtgs_keypoint_detect": len(kfs), "rtgs_keypoint_describe": len(kfs), "rtgs_keypoint_match": 1}
    assert all("init_source" not in c and "keypoints" not in c for c in reps["yaw"]["candidates"])


def test_strict_refuses_and_keypoints_falls_back_on_the_smooth_turn():
    """The smooth room has no corner in it: no keypoint, no match, no pose."""
    mapper, tracker, truth = mapped(turn_frames())
    truth_kf = [truth[i] for i in KEYFRAMES]
    before = state(mapper, tracker)
    out = lc.LoopCloser(loop_args(loop_closure_candidates="appearance", loop_closure_appearance_init="keypoints_strict")).close(mapper, tracker)
    print("strict:", brief(out))
    assert len(out["candidates"]) >= 3 and out["edges"] == 0 and out["changed"] is False
    for c in out["candidates"]:
        assert c["accepted"] is False and c["reason"] == f"keypoints: {c['keypoints']['inliers']} inliers of {c['keypoints']['matches']} matches, below 8"
        assert c["init_source"] == "yaw" and c["Z"] is None and all(c[k] is None for k in lc.REGISTER_FIGURES)
        assert set(c) == APPEARANCE_CANDIDATE_KEYS | {"init_source", "init", "keypoints"}
    after = state(mapper, tracker)
    assert np.array_equal(after[0], before[0]) and torch.equal(after[1], before[1]) and after[2] == before[2]
    out = lc.LoopCloser(loop_args(loop_closure_candidates="appearance", loop_closure_appearance_init="keypoints")).close(mapper, tracker)
    print("fallback:", brief(out))
    accepted = [c for c in out["candidates"] if c["accepted"]]
    assert all(c["init_source"] == "yaw" for c in out["candidates"]) and out["appearance"]["keypoint_inits"] == 0
    assert {(c["a"], c["b"]) for c in accepted} == {(0, 12), (1, 13), (2, 14)}               # the edges of today's appearance test
    for c in accepted:
        want = pg.inverse(truth_kf[c["a"]]) @ truth_kf[c["b"]]
        assert float(np.linalg.norm(np.asarray(c["Z"])[:3, 3] - want[:3, 3])) < 5e-3
    assert out["changed"] and out["edges"] == 3


@pytest.mark.parametrize("over", [dict(loop_closure_appearance_init="keypoints"),
                                  dict(loop_closure_candidates="pose", loop_closure_appearance_init="keypoints_strict"),
                                  dict(loop_closure_candidates="both", loop_closure_appearance_init="orb"),
                                  dict(loop_closure_candidates="both", loop_closure_appearance_init="keypoints", loop_closure_keypoint_cell=40),
                                  dict(loop_closure_keypoint_threshold=300), dict(loop_closure_keypoint_ratio=0.0),
                                  dict(loop_closure_keypoint_max_hamming=-1), dict(loop_closure_keypoint_ransac_iters=0),
                                  dict(loop_closure_keypoint_inlier_dist=-0.1), dict(loop_closure_keypoint_min_inliers=2)])
def test_invalid_values(over):
    with pytest.raises(ValueError):
        lc.LoopCloser(loop_args(**over))
    lc.LoopCloser(loop_args(loop_closure_candidates="both", loop_closure_appearance_init="keypoints", loop_closure_keypoint_cell=32,
                            loop_closure_keypoint_threshold=0, loop_closure_keypoint_ratio=1.0, loop_closure_keypoint_min_inliers=3,
                            loop_closure_keypoint_oriented=False))
