"""Map-quality evaluation on the MI355X (rtg_slam_amd.evaluation; include/rtgs_slam.h "evaluation"): the HIP picture and
reconstruction metrics against the float64 restatement of tests/eval_reference.py, their edge cases and run-to-run
determinism, and the two places the reference evaluates: the SLAM loop (run_sequence(eval_every=...)) and metric.py's
whole-sequence form (evaluate_sequence)."""
import math

import numpy as np
import pytest
import torch

from rtg_slam_amd import evaluation as ev, synth
from tests import eval_reference as er

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MIN_D, MAX_D = 0.3, 5.0


def _cam(H, W):
    return synth.CameraSpec(H, W, 0.5 * W, 0.5 * W, (W - 1) / 2, (H - 1) / 2)


def _render_inputs(H, W, seed):
    """A rasterizer render of a synthetic surface map against the box room's frame at the same pose; the GT depth gets
    pixels outside (min_depth, max_depth) on purpose, the render has depth_index == -1 pixels (the map is sparse)."""
    from rtg_slam_amd import mapping as mp
    from rtg_slam_amd.render import Renderer
    cam = _cam(H, W)
    c2w = synth.look_at_pose(seed=seed, max_angle_deg=20.0, max_trans=0.3)
    gs = {k: v.to(DEV) for k, v in synth.surface_gaussians(30000, cam, seed=seed).items()}
    frame = mp.Frame(cam, c2w.numpy(), DEV)
    with torch.no_grad():
        out = Renderer(mp.replica_args()).render(frame, gs)
    gt_depth = synth.box_room_depth(cam, c2w).reshape(H, W).to(DEV)
    gt_color = synth.box_room_color(cam, c2w, gt_depth.cpu()[..., None]).to(DEV)
    g = torch.Generator().manual_seed(seed)
    far = torch.rand(H, W, generator=g) < 0.03
    near = torch.rand(H, W, generator=g) < 0.03
    gt_depth = torch.where(far.to(DEV), torch.full_like(gt_depth, MAX_D + 1.0), gt_depth)
    gt_depth = torch.where(near.to(DEV), torch.full_like(gt_depth, 0.5 * MIN_D), gt_depth)
    gt_depth[0, :7] = MAX_D                                   # exactly on the bound: outside the open interval
    return out, gt_color, gt_depth


def _random_inputs(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=g)
    render = (gt + 0.08 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gt_depth = 0.1 + 6.0 * torch.rand(H, W, generator=g)
    depth = gt_depth[None] + 0.05 * torch.randn(1, H, W, generator=g)
    idx = torch.randint(-1, 1000, (1, H, W), generator=g, dtype=torch.int32)
    idx[torch.rand(1, H, W, generator=g) < 0.2] = -1
    out = {"render": render.to(DEV), "depth": depth.to(DEV), "depth_index_map": idx.to(DEV)}
    return out, gt.to(DEV), gt_depth.to(DEV)


def _check_picture(out, gt_color, gt_depth, tag):
    v = ev.picture_metrics(out["render"], gt_color, out["depth"], gt_depth, out["depth_index_map"], MIN_D, MAX_D).cpu().numpy()
    ref = er.picture(out["render"].cpu().numpy(), gt_color.cpu().numpy(), out["depth"].cpu().numpy(), gt_depth.cpu().numpy(),
                     out["depth_index_map"].cpu().numpy(), MIN_D, MAX_D)
    cs_d = np.abs(v[ev.OUT_CS:ev.OUT_CS + 15].reshape(5, 3) - ref["cs_levels"])
    ss_d = np.abs(v[ev.OUT_SSIM:ev.OUT_SSIM + 15].reshape(5, 3) - ref["ssim_levels"])
    t32 = er.ms_ssim_torch32(out["render"], gt_color)
    print(tag, "psnr", v[ev.OUT_PSNR], ref["psnr"], "ms_ssim", v[ev.OUT_MS_SSIM], ref["ssim"], "torch32", t32,
          "max |d cs| per level", cs_d.max(1), "max |d ssim| per level", ss_d.max(1))
    assert abs(v[ev.OUT_PSNR] - ref["psnr"]) <= 1e-4, tag
    assert abs(v[ev.OUT_COLOR_L1] - ref["color_l1"]) <= 1e-6 * ref["color_l1"], tag
    assert int(v[ev.OUT_VALID_COUNT]) == ref["valid_count"] and 0 < ref["valid_count"] < gt_depth.numel(), tag
    assert v[ev.OUT_VALID_RATIO] == ref["valid_pixel_ratio"], tag
    assert abs(v[ev.OUT_DEPTH_L1] - ref["depth_loss"]) <= 1e-6 * ref["depth_loss"], tag
    assert abs(v[ev.OUT_MS_SSIM] - ref["ssim"]) <= 1e-5, tag
    assert abs(v[ev.OUT_MS_SSIM] - t32) <= 1e-4, tag          # the float32 arithmetic the reference runs
    return v


@pytest.mark.parametrize("H,W", [(680, 1200), (480, 640), (341, 517)])
def test_picture_metrics_match_the_float64_restatement(H, W):
    out, gt_color, gt_depth = _render_inputs(H, W, seed=H)
    idx = out["depth_index_map"]
    assert bool((idx == -1).any()) and bool((idx != -1).any())
    _check_picture(out, gt_color, gt_depth, f"render {H}x{W}")
    _check_picture(*_random_inputs(H, W, seed=W), f"random {H}x{W}")
    # the dict form: the reference's keys, LPIPS not invented
    d = ev.eval_picture(out, gt_color, gt_depth, MIN_D, MAX_D)
    assert list(d) == ["valid_pixel_ratio", "depth_loss", "normal_loss", "psnr", "ssim", "lpips", "color_l1"]
    assert d["lpips"] is None and d["normal_loss"] == 0


def test_picture_edge_cases():
    H, W = 161, 300
    out, gt_color, gt_depth = _random_inputs(H, W, seed=7)
    # identical images: MS-SSIM 1, PSNR +inf (every channel's mse is 0)
    same = dict(out, render=gt_color.clone())
    d = ev.eval_picture(same, gt_color, gt_depth, MIN_D, MAX_D)
    assert abs(d["ssim"] - 1.0) <= 1e-6 and d["psnr"] == math.inf and d["color_l1"] == 0.0
    # no valid depth pixel: depth loss NaN, ratio 0
    none = dict(out, depth_index_map=torch.full_like(out["depth_index_map"], -1))
    d = ev.eval_picture(none, gt_color, gt_depth, MIN_D, MAX_D)
    assert math.isnan(d["depth_loss"]) and d["valid_pixel_ratio"] == 0.0
    d = ev.eval_picture(out, gt_color, torch.full_like(gt_depth, MAX_D + 1), MIN_D, MAX_D)
    assert math.isnan(d["depth_loss"]) and d["valid_pixel_ratio"] == 0.0
    # a 161-pixel side is accepted and matches the restatement
    _check_picture(out, gt_color, gt_depth, "random 161x300")
    with pytest.raises(ValueError):
        ev.eval_picture(dict(out, render=out["render"][:, :160], depth=out["depth"][:, :160],
                             depth_index_map=out["depth_index_map"][:, :160]), gt_color[:, :160], gt_depth[:160], MIN_D, MAX_D)


def _box_points(n, seed):
    """Points on the box room's walls (the GT side) and a noisy, partial copy (the reconstruction side)."""
    v = np.array([[x, y, z] for x in (-2.5, 2.5) for y in (-1.5, 1.5) for z in (-3.0, 3.0)], dtype=np.float64)
    q = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]])
    f = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])
    pts, _ = __import__("rtg_slam_amd.io_formats", fromlist=["x"]).sample_mesh_surface(v, f, n, seed=seed)
    return pts


def test_reconstruction_metrics_match_a_float64_brute_force():
    rng = np.random.default_rng(0)
    gt = torch.tensor(_box_points(30000, 1), dtype=torch.float32, device=DEV)
    rec_np = _box_points(28000, 2)
    rec_np = rec_np[rec_np[:, 0] < 2.0][:20000] + 0.02 * rng.standard_normal((20000, 3))   # one wall missing: recall < 100 %
    rec = torch.tensor(rec_np, dtype=torch.float32, device=DEV)
    thres = (0.01, 0.03, 0.05)
    T = np.eye(4)
    T[:3, :3] = synth.se3_exp(torch.tensor([0.02, -0.01, 0.03, 0.0, 0.0, 0.0], dtype=torch.float64))[:3, :3].numpy()
    T[:3, 3] = [0.01, -0.02, 0.005]
    for transform in (None, T):
        res = ev.eval_pcd(rec, gt, thres, transform=transform)
        r64 = rec.double()
        if transform is not None:
            Tt = torch.tensor(transform, dtype=torch.float64, device=DEV)
            r64 = r64 @ Tt[:3, :3].t() + Tt[:3, 3]
        d_acc = er.nn_distances(r64, gt.double())
        d_comp = er.nn_distances(gt.double(), r64)
        print("transform" if transform is not None else "identity", res)
        assert abs(res["accuracy"] / 100 - float(d_acc.mean())) <= 1e-6
        assert abs(res["completion"] / 100 - float(d_comp.mean())) <= 1e-6
        for t in thres:
            for key, d, n in (("P", d_acc, rec.shape[0]), ("R", d_comp, gt.shape[0])):
                want = int((d < t).sum())
                slack = int(((d - t).abs() <= 1e-6).sum())
                got = res[f"{key} (< {t})"] * n / 100
                assert abs(round(got) - want) <= slack, (key, t, got, want, slack)
            P, R = res[f"P (< {t})"], res[f"R (< {t})"]
            assert abs(res[f"F1 (< {t})"] - 2 * P * R / (P + R)) < 1e-9
        assert 0 < res["R (< 0.05)"] < 100
    # bitwise reproducible, and the sub-sample has the requested size and follows the generator
    a = ev.eval_pcd(rec, gt, thres, transform=T, sample_nums=5000, generator=torch.Generator().manual_seed(3))
    b = ev.eval_pcd(rec, gt, thres, transform=T, sample_nums=5000, generator=torch.Generator().manual_seed(3))
    assert a == b
    s1 = ev.subsample(rec, 5000, torch.Generator().manual_seed(3))
    s2 = ev.subsample(rec, 5000, torch.Generator().manual_seed(3))
    assert s1.shape == (5000, 3) and torch.equal(s1, s2)
    assert torch.unique(s1, dim=0).shape[0] == 5000
    assert ev.subsample(rec, 10 ** 6) is rec
    # F1 of disjoint sets: P = R = 0 -> NaN, as the reference's division
    far = ev.eval_pcd(rec + 100.0, gt, (0.03,))
    assert far["P (< 0.03)"] == 0 and far["R (< 0.03)"] == 0 and math.isnan(far["F1 (< 0.03)"])


def test_metrics_are_bitwise_reproducible():
    out, gt_color, gt_depth = _render_inputs(680, 1200, seed=5)
    args = (out["render"], gt_color, out["depth"], gt_depth, out["depth_index_map"], MIN_D, MAX_D)
    v1, v2 = ev.picture_metrics(*args), ev.picture_metrics(*args)
    assert torch.equal(v1.view(torch.int64), v2.view(torch.int64))
    g = torch.rand(200000, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    d2 = torch.rand(200000, 3, generator=torch.Generator().manual_seed(2)).to(DEV) * 0.01
    thr = torch.tensor([0.01, 0.05, 0.08], dtype=torch.float64, device=DEV)
    n1, n2 = ev.nn_stats(d2, thr), ev.nn_stats(d2, thr)
    assert torch.equal(n1.view(torch.int64), n2.view(torch.int64))
    assert int(n1[3]) == int((d2[:, 0].double().sqrt() < 0.08).sum())
    assert abs(float(n1[0]) - float(d2[:, 0].double().sqrt().sum())) < 1e-9 * float(n1[0])
    p1, p2 = ev.eval_pcd(g, g[::2] + 0.001, (0.01, 0.03)), ev.eval_pcd(g, g[::2] + 0.001, (0.01, 0.03))
    assert p1 == p2


# ------------------------------------------------------------------------------------------------ in the loop / metric.py
def _half_replica():
    c = synth.REPLICA
    return synth.CameraSpec(c.H // 2, c.W // 2, c.fx / 2, c.fy / 2, (c.cx + 0.5) / 2 - 0.5, (c.cy + 0.5) / 2 - 0.5)


def _frames(cam, n, seed=21):
    out = []
    for p in synth.trajectory(n, seed=seed):
        d = synth.box_room_depth(cam, p)
        out.append((d.to(DEV), synth.box_room_color(cam, p, d).to(DEV), p.numpy()))
    return out


def _args():
    from rtg_slam_amd import mapping as mp
    return mp.replica_args(uniform_sample_num=10200, gaussian_update_iter=30, stable_confidence_thres=40.0,
                           unstable_time_window=24, max_depth=8.0, keyframe_trans_thes=0.25, seed=1)


@pytest.fixture(scope="module")
def evaluated_run():
    from rtg_slam_amd import mapping as mp, slam
    cam = _half_replica()
    frames = _frames(cam, 30)
    args = _args()
    mapper = mp.Mapping(args, DEV, capacity=200_000)
    mapper, tracker, rep = slam.run_sequence(cam, iter(frames), args, DEV, mapper=mapper, final_global=True, eval_every=10)
    return cam, frames, args, mapper, tracker, rep


OLD_REPORT_KEYS = ["frames", "tracking_s_mean", "mapping_s_mean", "fps", "fps_tracking_plus_mapping", "wall_s", "ate_rmse_m",
                   "ate_rmse_aligned_m", "final_translation_error_m", "gaussians", "stable", "unstable", "keyframes", "stats",
                   "stable_fraction_over_time", "gaussians_over_time", "per_frame", "stage_profile_ms_per_frame"]


def test_run_sequence_evaluates_at_the_references_frames(evaluated_run):
    from rtg_slam_amd import mapping as mp, slam
    cam, frames, args, mapper, tracker, rep = evaluated_run
    rows = rep["eval"]
    for r in rows:
        print({k: r[k] for k in ("frame", "final", "psnr", "ssim", "depth_loss", "valid_pixel_ratio", "color_l1")})
    assert [(r["frame"], r["final"]) for r in rows[:-1]] == [(0, False), (9, False), (19, False), (29, False)]
    assert rows[-1]["final"] and rows[-1]["frame"] == mapper.keyframe_ids[-1]
    for r in rows:
        assert r["psnr"] > 24.0 and r["depth_loss"] < 0.02 and 0.5 < r["ssim"] <= 1.0 and r["lpips"] is None
    assert list(rep)[:-1] == OLD_REPORT_KEYS and list(rep)[-1] == "eval"
    # without eval_every: exactly the keys the report always had
    _, _, rep0 = slam.run_sequence(cam, iter(frames[:3]), args, DEV, mapper=mp.Mapping(args, DEV, capacity=200_000))
    assert list(rep0) == OLD_REPORT_KEYS


def test_evaluate_sequence_is_metric_py(evaluated_run, tmp_path):
    """metric.py's form on the map of the evaluated run, GT points back-projected from the stream's GT depth.
    Bounds: accuracy < 2 cm, F1 (< 3 cm) > 80 %.  Measured on the MI355X at the first run: accuracy 0.59 cm, completion
    2.05 cm, P / R (< 3 cm) 99.8 / 84.9 %, F1 (< 3 cm) 91.7 %; mean PSNR 51.1 dB, MS-SSIM 0.999, depth L1 0.49 cm."""
    from rtg_slam_amd import io_formats as iof
    cam, frames, args, mapper, tracker, rep = evaluated_run
    pts = []
    ys, xs = torch.meshgrid(torch.arange(cam.H, device=DEV, dtype=torch.float64),
                            torch.arange(cam.W, device=DEV, dtype=torch.float64), indexing="ij")
    for depth, _, c2w in frames[::3]:
        z = depth.reshape(cam.H, cam.W).double()
        pc = torch.stack([(xs - cam.cx) / cam.fx * z, (ys - cam.cy) / cam.fy * z, z], -1)[z > 0]
        T = torch.tensor(c2w, dtype=torch.float64, device=DEV)
        pts.append((pc @ T[:3, :3].t() + T[:3, 3])[::7])
    gt_points = torch.cat(pts).float()
    res = ev.evaluate_sequence(mapper, cam, iter(frames), poses=tracker.pose_es, gt_points=gt_points,
                               dist_thres=(0.01, 0.03), generator=torch.Generator().manual_seed(0))
    rows, mean = res["rows"], res["mean"]
    print("mean", mean)
    assert [r["frame"] for r in rows] == list(range(len(frames)))
    assert mean["frame"] == "mean" and abs(mean["psnr"] - np.mean([r["psnr"] for r in rows])) < 1e-9
    assert "accuracy" in rows[-1] and "accuracy" not in rows[0] and mean["accuracy"] == rows[-1]["accuracy"]
    assert mean["psnr"] > 24.0 and mean["depth_loss"] < 0.02
    assert rows[-1]["accuracy"] < 2.0 and rows[-1]["F1 (< 0.03)"] > 80.0
    # GT poses instead of the estimated ones: the same frames, close values (ATE < 1 cm on this stream)
    res_gt = ev.evaluate_sequence(mapper, cam, iter(frames[:3]))
    assert [r["frame"] for r in res_gt["rows"]] == [0, 1, 2]
    assert abs(res_gt["rows"][0]["psnr"] - rows[0]["psnr"]) < 1.0
    iof.save_metrics_csv(str(tmp_path / "statis.csv"), rows)
    assert (tmp_path / "statis.csv").read_text().splitlines()[-1].split(",")[1] != ""
