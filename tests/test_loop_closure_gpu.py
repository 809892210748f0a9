"""rtg_slam_amd/loop_closure.py end to end: a loop in the box room mapped along a drifting trajectory, closed by LoopCloser.close;
and the option switched off, or on without a candidate, changing nothing.

The loop: a camera near the room's centre yaws through a full turn in FRAMES steps at 320 x 240; gaussian_update_frame 3 and
keyframe_theta_thes 15 make every third frame a keyframe.  The mapper runs at use_gt_pose on a stream whose poses carry an injected drift that grows linearly,
pose_k = exp(k DRIFT) T_k with D_0 = I, so that it builds the doubled wall a real drift builds where the turn closes.

DRIFT and FRAMES were chosen on the CPU (`python -m tests.test_loop_closure_gpu` repeats it): starting from 1.5 mm and 0.03 degrees
per frame, the largest multiple in (1, 1.5, 2, 3, 4) at which tests/rgbd_align_reference.refine registers the last keyframe onto the
first from the drifted guess - every gate of loop_closure.register_pair passed and the result within 5 mm of the truth.  That
is 3: the guess is then off by 160 mm and 3.15 degrees at the last keyframe and the reference ends 0.19 mm from the truth (inlier
ratio 0.819, rms 0.3 mm); at 4 the registration still lands there, but its 214 mm exceed loop_closure_max_correction_trans.

The loop edges are weighted 2 000 times the odometry edges: an odometry edge of this stream is wrong by 3 frames of drift, 13.5
mm, a registration of these noise-free frames by 0.2 - 0.3 mm, and the weights are inverse variances: (13.5 / 0.3)^2."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import pose_graph as pg
from rtg_slam_amd import synth
from rtg_slam_amd.rgbd_align import se3_exp, se3_log

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CAM = synth.CameraSpec(240, 320, 160.0, 160.0, 159.5, 119.5)
FRAMES = 36                                                     # 10 degrees a frame
KEYFRAMES = [0] + list(range(2, FRAMES, 3))                     # the mapper looks at frame 0 and then at every third: 13 keyframes
CENTRE = (0.15, -0.1, 0.2)
UNIT = np.array([0.0, np.deg2rad(0.03) * 0.8, np.deg2rad(0.03) * 0.6, 0.0015 * 0.6, 0.0, 0.0015 * 0.8])
SCALE = 3.0                                                     # the chosen multiple: 4.5 mm and 0.09 degrees per frame
DRIFT = SCALE * UNIT


def true_poses(n=FRAMES):
    out = []
    for k in range(n):
        T = se3_exp([0.0, 2 * np.pi * k / n, 0.0, 0.0, 0.0, 0.0])
        T[:3, 3] = CENTRE
        out.append(T)
    return out


def drifted_poses(truth, drift=DRIFT):
    return [se3_exp(k * np.asarray(drift)) @ T for k, T in enumerate(truth)]


def loop_args(**over):
    from rtg_slam_amd import mapping as mp
    kw = dict(uniform_sample_num=4000, gaussian_update_iter=10, max_depth=8.0, keyframe_theta_thes=15.0, keyframe_trans_thes=10.0,
              gaussian_update_frame=3,
              seed=1, use_gt_pose=True, loop_closure_max_rot_deg=35.0, loop_closure_loop_weights=[2000.0, 2000.0])
    kw.update(over)
    return mp.replica_args(**kw)


_frames = {}


def frames(n=FRAMES):
    """(depth, colour, true c2w) of the turn, rendered once."""
    if n not in _frames:
        out = []
        for T in true_poses(n):
            p = torch.from_numpy(T)
            d = synth.box_room_depth(CAM, p)
            out.append((d.to(DEV), synth.box_room_color(CAM, p, d).to(DEV), T))
        _frames[n] = out
    return _frames[n]


def depth_error(mapper, truth_kf, depths):
    """Mean |rendered depth - true depth| at the TRUE keyframe poses, over the pixels valid in both."""
    from rtg_slam_amd.mapping import Frame
    tot, cnt = 0.0, 0
    for T, d in zip(truth_kf, depths):
        out = mapper._render(Frame(CAM, T, DEV), "all")
        r, g = out["depth"].reshape(CAM.H, CAM.W), d.reshape(CAM.H, CAM.W)
        ok = (r > 0) & (g > 0)
        tot += float((r - g).abs()[ok].sum())
        cnt += int(ok.sum())
    return tot / max(cnt, 1)


def kf_rms(poses, truth):
    return float(np.sqrt(np.mean([np.sum((p[:3, 3] - t[:3, 3]) ** 2) for p, t in zip(poses, truth)])))


def test_a_drifted_loop_is_closed():
    """Measured on an MI355X: both candidates, (1, 12) and (0, 12), are accepted (inlier ratios 0.595 and 0.819, rms 0.2 and 0.3
    mm, corrections 151 and 160 mm); the keyframes' rms translation error against the TRUE poses falls from 93.19 mm to 0.19 mm,
    the mean depth error of the map rendered at the true keyframe poses from 43.43 mm to 13.35 mm (what stays is the part of
    the doubled wall whose rows moved with the wrong one of two overlapping frames, and the map's own error); the whole closure
    takes 24 ms, 16 of them in the graph."""
    from rtg_slam_amd import slam
    fr = frames()
    truth = [f[2] for f in fr]
    drifted = drifted_poses(truth)
    args = loop_args()
    torch.manual_seed(1)
    stream = ((d, c, drifted[k]) for k, (d, c, _) in enumerate(fr))
    mapper, tracker, rep = slam.run_sequence(CAM, stream, args, DEV, capacity=200_000)
    assert "loop_closure" not in rep
    ids = list(mapper.keyframe_ids)
    assert ids == KEYFRAMES, ids
    truth_kf, depths = [truth[i] for i in ids], [fr[i][0] for i in ids]
    rms_before = kf_rms([tracker.pose_es[i] for i in ids], truth_kf)
    depth_before = depth_error(mapper, truth_kf, depths)
    normals_before = [km["normal_map_w"].clone() for km in mapper.keymap_list]
    version = mapper.opt.version
    closer = lc.LoopCloser(args)
    out = closer.close(mapper, tracker)
    M = len(ids)
    accepted = [(c["a"], c["b"]) for c in out["candidates"] if c["accepted"]]
    print("candidates:", [(c["a"], c["b"], c["reason"], round(c["inlier_ratio"], 3), round(c["rms_geometric_after"], 4),
                           round(c["correction_trans"], 4)) for c in out["candidates"]])
    assert any(a < 3 and b >= M - 3 for a, b in accepted), out["candidates"]
    assert out["changed"] and out["edges"] == len(accepted) and mapper.opt.version > version
    rms_after = kf_rms([tracker.pose_es[i] for i in ids], truth_kf)
    depth_after = depth_error(mapper, truth_kf, depths)
    print(f"keyframe rms translation error {1e3 * rms_before:.2f} -> {1e3 * rms_after:.2f} mm; depth error at the true keyframe "
          f"poses {1e3 * depth_before:.2f} -> {1e3 * depth_after:.2f} mm; ATE against the true poses "
          f"{1e3 * slam.ate_rmse(drifted, truth):.2f} -> {1e3 * slam.ate_rmse(tracker.pose_es, truth):.2f} mm; largest correction "
          f"{1e3 * out['correction_max_m']:.2f} mm; seconds {out['seconds']}")
    assert rms_after < 0.5 * rms_before
    assert depth_after < depth_before
    assert slam.ate_rmse(tracker.pose_es, truth) < 0.5 * slam.ate_rmse(drifted, truth)
    # the report's own ATE is against what the stream called ground truth - here the drifted poses the run was fed
    assert out["ate_rmse_m_before"] == 0.0 and abs(out["ate_rmse_m"] - slam.ate_rmse(tracker.pose_es, drifted)) < 1e-12
    # the keyframes' frames and kept normals moved with the poses; frame 0 is held
    for k, kf in enumerate(mapper.keyframe_list):
        assert np.array_equal(kf.c2w.numpy(), tracker.pose_es[ids[k]])
    assert np.array_equal(tracker.pose_es[0], drifted[0])
    assert torch.equal(mapper.keymap_list[0]["normal_map_w"], normals_before[0])
    assert not torch.equal(mapper.keymap_list[-1]["normal_map_w"], normals_before[-1])
    # a second closure finds nothing left to correct
    again = closer.close(mapper, tracker)
    print(f"second closure: {again['edges']} edges, largest correction {1e3 * again.get('correction_max_m', 0.0):.3f} mm")
    assert again["edges"] >= 1 and again["correction_max_m"] < 1e-3


# ---- off means off ----

def straight_stream(n=6):
    for k, p in enumerate(synth.trajectory(n, seed=21)):
        d = synth.box_room_depth(CAM, p)
        yield d.to(DEV), synth.box_room_color(CAM, p, d).to(DEV), p.numpy()


def test_off_means_off(monkeypatch):
    """As tests/test_map_exposure_gpu.py: gaussian_update_iter = 0 makes two runs of the same arguments bit-reproducible."""
    from rtg_slam_amd import _lib, slam
    lib = _lib.load()
    calls = [0]
    real = lib.rtgs_map_deform

    def counted(*a):
        calls[0] += 1
        return real(*a)
    monkeypatch.setattr(lib, "rtgs_map_deform", counted)
    runs = {}
    for name, over in (("absent", {}), ("false", {"loop_closure": False}), ("on", {"loop_closure": True})):
        args = loop_args(gaussian_update_iter=0, keyframe_trans_thes=0.01, **over)
        torch.manual_seed(1)
        runs[name] = slam.run_sequence(CAM, straight_stream(), args, DEV, capacity=100_000, final_global=False)
    m_a, t_a, rep_a = runs["absent"]
    assert not hasattr(loop_args(), "loop_closure") and "loop_closure" not in rep_a and "loop_closure" not in runs["false"][2]
    assert not hasattr(t_a, "pose_es_before_loop_closure")
    assert m_a.opt.N > 4000 and len(m_a.keyframe_ids) >= 3                      # keyframes there are, none ten keyframes apart
    rep = runs["on"][2]["loop_closure"]
    print("on without a candidate:", {k: rep[k] for k in ("keyframes", "edges", "changed")}, len(rep["candidates"]))
    assert rep["edges"] == 0 and not rep["changed"] and rep["candidates"] == []     # a short straight stream: no pair lies close
    assert calls[0] == 0
    for name in ("false", "on"):
        m, t, _ = runs[name]
        assert np.array_equal(np.stack(t.pose_es), np.stack(t_a.pose_es))
        assert m.opt.N == m_a.opt.N and torch.equal(m.opt.params[:m.opt.N], m_a.opt.params[:m_a.opt.N])
        assert m.opt.version == m_a.opt.version
    assert np.array_equal(np.stack(runs["on"][1].pose_es_before_loop_closure), np.stack(t_a.pose_es))


def test_refusals():
    from rtg_slam_amd import slam
    with pytest.raises(ValueError):
        slam.run_sequence(CAM, straight_stream(2), loop_args(loop_closure=True, loop_closure_min_gap=0), DEV, capacity=50_000)


# ---- the choice of DRIFT, on the CPU ----

def choose_drift():
    from oracle import icp_oracle as io
    from tests import rgbd_align_reference as ref
    K = torch.tensor([[CAM.fx, 0, CAM.cx], [0, CAM.fy, CAM.cy], [0, 0, 1]], dtype=torch.float32)
    truth = true_poses()
    a, b = KEYFRAMES[0], KEYFRAMES[-1]                          # the first and the last keyframe
    maps = []
    for k in (a, b):
        p = torch.from_numpy(truth[k])
        d = synth.box_room_depth(CAM, p)
        vp = io.vertex_pyramid(d, K, 3)
        maps.append(([x.numpy() for x in vp], [x.numpy() for x in io.normal_pyramid(vp)],
                     ref.intensity_pyramid(synth.box_room_color(CAM, p, d).numpy(), 3)))
    want = pg.inverse(truth[a]) @ truth[b]
    cfg = lc.LoopCloser(loop_args()).cfg
    for scale in (1, 1.5, 2, 3, 4):
        guess = pg.inverse(truth[a]) @ se3_exp(b * scale * UNIT) @ truth[b]
        Z, rep = ref.refine(guess, *maps[1], *maps[0], K.numpy(), [0.25, 0.5, 1.0], distance_threshold=0.1,
                            cos_threshold=float(np.cos(np.deg2rad(20.0))))
        valid = int((maps[1][0][-1][..., 2] > 0).sum())
        C = pg.inverse(guess) @ Z
        ok = (rep["reason"] == "done" and min(rep["rank"]) == 6 and rep["inliers_geometric"][-1] / valid >= cfg.min_inlier_ratio
              and rep["rms_geometric_after"] <= cfg.max_rms and np.linalg.norm(C[:3, 3]) <= cfg.max_correction_trans)
        err = np.linalg.norm(Z[:3, 3] - want[:3, 3])
        print(f"scale {scale}: guess off by {1e3 * np.linalg.norm(guess[:3, 3] - want[:3, 3]):.1f} mm / "
              f"{np.rad2deg(np.linalg.norm(se3_log(pg.inverse(want) @ guess)[:3])):.2f} degrees -> {1e3 * err:.2f} mm, gates "
              f"{'pass' if ok else 'fail'} (inliers {rep['inliers_geometric'][-1] / valid:.3f}, rms {rep['rms_geometric_after']:.4f}, "
              f"{rep['reason']}, rank {min(rep['rank']) if rep['rank'] else 0})")


if __name__ == "__main__":
    choose_drift()
