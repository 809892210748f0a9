"""rtg_slam_amd/relocalisation.py end to end, 320 x 240, the textured box room, use_gt_pose False.

THE STREAM (tests/test_relocalisation_cpu.py checks its precondition from the definitions alone):
    part A   30 frames turning 1 degree a frame at CENTRE; gaussian_update_frame 3 and keyframe_theta_thes 1.5 make the keyframes
             [0, 2, 5, .., 29]
    part B   4 covered frames, depth and colour all zero: ICP reports singular normal equations through its status word
    part C   16 frames from the view 3 degrees and (0.04, -0.02, 0.03) m beside the yaw-11 view, turning 1 degree a frame onwards
With the option on the covered frames are lost and frame 34 is recovered from the keyframes; today's tree raises in predict_pose
at frame 30."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import relocalisation as rl
from rtg_slam_amd import slam, synth
from tests.test_keypoints_cpu import RIGHT, textured_view, view_pose
from tests.test_loop_closure_gpu import CAM, DEV, loop_args
from tests.test_place_cpu import angle_deg

pytestmark = pytest.mark.gpu
PART_A, COVERED, PART_C = 30, 4, 16
RETURN_YAW, RETURN_OFFSET = 11.0 + RIGHT["54 mm / 3 deg"][0], RIGHT["54 mm / 3 deg"][1]
KEYFRAMES_A = [0] + list(range(2, PART_A, 3))
KERNELS = ("rtgs_place_describe", "rtgs_place_scores", "rtgs_keypoint_detect", "rtgs_keypoint_describe", "rtgs_keypoint_match",
           "rtgs_rigid_ransac")


def reloc_args(**over):
    return loop_args(**dict(dict(use_gt_pose=False, gaussian_update_iter=3, keyframe_theta_thes=1.5), **over))


def part_a_poses(n=PART_A):
    return [view_pose(float(k)) for k in range(n)]


def part_c_poses(n=PART_C):
    return [view_pose(RETURN_YAW + k, RETURN_OFFSET) for k in range(n)]


def textured(T):
    d, c = textured_view(T)
    return d.to(DEV), c.to(DEV), T


def covered(T):
    return torch.zeros((CAM.H, CAM.W, 1), device=DEV), torch.zeros((3, CAM.H, CAM.W), device=DEV), T


def smooth(T):
    p = torch.from_numpy(T)
    d = synth.box_room_depth(CAM, p)
    return d.to(DEV), synth.box_room_color(CAM, p, d).to(DEV), T


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


def trans_err(p, t):
    return float(np.linalg.norm(np.asarray(p)[:3, 3] - np.asarray(t)[:3, 3]))


def test_the_covered_frames_are_lost_and_the_return_frame_is_recovered():
    """Measured on an MI355X: frames 30 .. 33 lost (four times "no keyframe above the score": the best of 11 is -1, a black frame
    has no variance); recovered at frame 34 from keyframe 5 (frame 14): score 0.9873, 85 matches, 81 inliers - the definitions'
    figures of tests/test_relocalisation_cpu.py - correction 4.05 mm / 0.079 degrees; error 0.62 mm (the keyframe's 0.68 mm /
    0.008 degrees, arm 53.8 mm: bound 5.68 mm); part A at most 1.10 mm, part C at most 1.50 mm (bound 6.79 mm); keyframes 11 -> 16;
    ATE over the tracked frames 0.96 mm, over all 0.97 mm.  Seconds of the five attempts together: describe 1.1 ms, scores 0.5 ms,
    keypoints 29 ms (the process's first launches), match 0.17 ms, RANSAC 0.56 ms, registration 2.3 ms."""
    A, C = part_a_poses(), part_c_poses()
    truth = A + [A[-1]] * COVERED + C
    stream = [textured(T) for T in A] + [covered(A[-1])] * COVERED + [textured(T) for T in C]
    sizes, kfs = [], []

    def on_frame(frame_id, frame, frame_map, mapper, tracker):
        sizes.append(int(mapper.opt.N))
        kfs.append(len(mapper.keyframe_ids))
    torch.manual_seed(1)
    mapper, tracker, rep = slam.run_sequence(CAM, iter(stream), reloc_args(relocalise=True), DEV, capacity=200_000, on_frame=on_frame)
    lost = list(range(PART_A, PART_A + COVERED))
    first_c = PART_A + COVERED
    r = rep["relocalisation"]
    print("relocalisation:", {k: v for k, v in r.items() if k != "events"}, [{k: v for k, v in e.items() if k != "Z"} for e in r["events"]])
    assert tracker.lost_frames == lost and r["lost_frames"] == lost
    assert len(tracker.pose_es) == len(stream) == int(mapper.time)
    for f in lost:                                                # the pose of frame 29, no Gaussian and no keyframe added
        assert np.array_equal(tracker.pose_es[f], tracker.pose_es[PART_A - 1])
        assert sizes[f] == sizes[PART_A - 1] and kfs[f] == kfs[PART_A - 1]
    assert list(mapper.keyframe_ids)[:len(KEYFRAMES_A)] == KEYFRAMES_A and kfs[PART_A - 1] == len(KEYFRAMES_A)
    assert len(r["events"]) == 1 and r["attempts"] == COVERED + 1
    e = r["events"][0]
    assert (e["lost_at"], e["recovered_at"]) == (PART_A, first_c) and e["inliers"] >= 8
    assert r["refusals"] == {"no keyframe above the score": COVERED}
    # the recovered frame: at most its keyframe's own error, the registration's 5 mm, and the keyframe's rotation error on Z's arm
    kf_frame = e["keyframe_frame"]
    kf_err = trans_err(tracker.pose_es[kf_frame], truth[kf_frame])
    kf_rot = np.deg2rad(angle_deg(np.linalg.inv(truth[kf_frame]) @ tracker.pose_es[kf_frame]))
    arm = float(np.linalg.norm(np.asarray(e["Z"])[:3, 3]))
    bound = kf_err + 5e-3 + kf_rot * arm
    err = trans_err(tracker.pose_es[first_c], truth[first_c])
    worst_a = max(trans_err(tracker.pose_es[k], truth[k]) for k in range(PART_A))
    worst_c = max(trans_err(tracker.pose_es[k], truth[k]) for k in range(first_c, len(stream)))
    print(f"recovered at frame {first_c} from keyframe {e['keyframe']} (frame {kf_frame}): score {e['score']:.4f}, {e['matches']} matches, "
          f"{e['inliers']} inliers, correction {1e3 * e['correction_trans']:.2f} mm / {e['correction_rot_deg']:.3f} deg; error "
          f"{1e3 * err:.2f} mm (keyframe {1e3 * kf_err:.2f} mm / {np.rad2deg(kf_rot):.3f} deg, arm {1e3 * arm:.1f} mm, bound {1e3 * bound:.2f} mm); "
          f"part A at most {1e3 * worst_a:.2f} mm, part C at most {1e3 * worst_c:.2f} mm (bound {1e3 * (bound + worst_a):.2f} mm); "
          f"keyframes {kfs[PART_A - 1]} -> {kfs[-1]}; ATE tracked {1e3 * rep['ate_rmse_tracked_m']:.2f} mm, all frames {1e3 * rep['ate_rmse_m']:.2f} mm; "
          f"seconds {({k: round(v, 5) for k, v in r['seconds'].items()})}")
    assert err <= bound
    assert worst_c <= bound + worst_a
    assert kfs[-1] > kfs[PART_A - 1] and sizes[-1] > sizes[PART_A - 1]
    kept = [k for k in range(len(stream)) if k not in lost]
    assert rep["ate_rmse_tracked_m"] == slam.ate_rmse([tracker.pose_es[k] for k in kept], [truth[k] for k in kept])


def test_today_the_stream_raises():
    A = part_a_poses(6)
    stream = [textured(T) for T in A] + [covered(A[-1])]
    torch.manual_seed(1)
    with pytest.raises(RuntimeError, match="singular normal equations"):
        slam.run_sequence(CAM, iter(stream), reloc_args(), DEV, capacity=100_000)


def test_a_frame_that_cannot_be_recovered_stays_lost():
    """The covered frames followed by views of the smooth room, which has no corner: every one stays lost, the map is untouched.
    Measured on an MI355X: refusals {"no keyframe above the score": 2, "no keypoints": 5}."""
    A = part_a_poses(12)
    after = [view_pose(11.0 + k) for k in range(5)]
    stream = [textured(T) for T in A] + [covered(A[-1])] * 2 + [smooth(T) for T in after]
    state = []

    def on_frame(frame_id, frame, frame_map, mapper, tracker):
        state.append((int(mapper.opt.N), int(mapper.opt.version), len(mapper.keyframe_ids)))
    torch.manual_seed(1)
    mapper, tracker, rep = slam.run_sequence(CAM, iter(stream), reloc_args(relocalise=True), DEV, capacity=100_000, on_frame=on_frame)
    r = rep["relocalisation"]
    print("stays lost:", r["refusals"], r["last_refusal"])
    assert tracker.lost_frames == list(range(12, 19)) and r["events"] == [] and r["attempts"] == 7 and tracker.lost
    assert sum(r["refusals"].values()) == 7 and r["refusals"]["no keyframe above the score"] >= 2
    assert all(s == state[11] for s in state[12:])
    assert all(np.array_equal(tracker.pose_es[k], tracker.pose_es[11]) for k in range(12, 19)) and int(mapper.time) == 19


def test_off_means_off(monkeypatch):
    """gaussian_update_iter 0, as in the other off-means-off tests: the optimiser's float atomics make two runs of one tree differ
    in the last bits, and this test is about the option, not about them."""
    calls = count_kernels(monkeypatch)
    A = part_a_poses(9)
    runs = {}
    for name, over in (("absent", {}), ("false", {"relocalise": False}), ("on", {"relocalise": True})):
        torch.manual_seed(1)
        before = dict(calls)
        runs[name] = slam.run_sequence(CAM, iter([textured(T) for T in A]), reloc_args(gaussian_update_iter=0, **over), DEV, capacity=100_000)
        spent = {k: calls[k] - before[k] for k in calls}
        if name == "on":
            assert spent == dict({k: 0 for k in KERNELS}, rtgs_place_describe=len(runs[name][0].keyframe_ids)), spent
        else:
            assert spent == {k: 0 for k in KERNELS}, spent
            assert "relocalisation" not in runs[name][2] and "ate_rmse_tracked_m" not in runs[name][2]
    assert list(runs["on"][0].keyframe_ids) == [0, 2, 5, 8]
    rep = runs["on"][2]["relocalisation"]
    assert rep["lost_frames"] == [] and rep["attempts"] == 0 and rep["events"] == [] and rep["refusals"] == {} and rep["keyframes_described"] == 4
    assert runs["on"][2]["ate_rmse_tracked_m"] == runs["on"][2]["ate_rmse_m"]
    ref_m, ref_t, _ = runs["absent"]
    for name in ("false", "on"):
        m, t, _ = runs[name]
        assert np.array_equal(np.stack(t.pose_es), np.stack(ref_t.pose_es)), name
        assert m.opt.N == ref_m.opt.N and torch.equal(m.opt.params[:m.opt.N], ref_m.opt.params[:ref_m.opt.N]), name


def never():
    raise AssertionError("the stream was read")
    yield


@pytest.mark.parametrize("over,error", [(dict(relocalise_candidates=0), ValueError), (dict(relocalise_min_score=2.0), ValueError),
                                        (dict(relocalise_max_depth_rel=-0.1), ValueError), (dict(relocalise_thumb_width=0), ValueError),
                                        (dict(relocalise_max_shift=20), ValueError), (dict(relocalise_min_inliers=2), ValueError),
                                        (dict(relocalise_max_rms=-1.0), ValueError), (dict(relocalise_min_inlier_ratio=1.5), ValueError),
                                        (dict(use_gt_pose=True), ValueError)])
def test_bad_values_stop_the_run_before_its_first_frame(over, error):
    with pytest.raises(error):
        slam.run_sequence(CAM, never(), reloc_args(**dict(dict(relocalise=True), **over)), DEV, capacity=1000)


def test_the_two_refusals():
    with pytest.raises(RuntimeError, match="one rank"):
        rl.Relocaliser(reloc_args(relocalise=True), world=2)
    with pytest.raises(ValueError, match="pipeline"):
        rl.refuse_pipeline(reloc_args(relocalise=True))
    rl.refuse_pipeline(reloc_args())
    rl.refuse_pipeline(reloc_args(relocalise=False))
    slam.run_sequence(CAM, iter(()), reloc_args(relocalise=True, relocalise_candidates=1, relocalise_min_score=0.8), DEV, capacity=1000)
