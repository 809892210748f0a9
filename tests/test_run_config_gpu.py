"""End to end: `python -m rtg_slam_amd slam` and `metric` on a Replica-layout dataset written to disk (u16 depth PNGs at
scale 6553.5, JPEG colour) from the synthetic box room, with a config whose parent chain is the committed copies of the
reference's files; then the metric CSV against an in-process evaluate_sequence of the same saved map."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from rtg_slam_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
N = 20


def _half_replica():
    c = synth.REPLICA
    return synth.CameraSpec(c.H // 2, c.W // 2, c.fx / 2, c.fy / 2, (c.cx + 0.5) / 2 - 0.5, (c.cy + 0.5) / 2 - 0.5)


def _write_dataset(root):
    cam = _half_replica()
    scene = os.path.join(root, "Replica", "room0")
    os.makedirs(os.path.join(scene, "results"))
    lines = []
    for i, p in enumerate(synth.trajectory(N, seed=21)):
        d = synth.box_room_depth(cam, p)
        col = synth.box_room_color(cam, p, d)
        raw = np.clip(np.round(d[..., 0].double().numpy() * 6553.5), 0, 65535).astype(np.uint16)
        Image.fromarray(raw).save(os.path.join(scene, "results", f"depth{i:06d}.png"))
        rgb = np.clip(np.round(col.permute(1, 2, 0).double().numpy() * 255), 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(os.path.join(scene, "results", f"frame{i:06d}.jpg"), quality=95)
        lines.append(" ".join(repr(float(v)) for v in p.numpy().reshape(-1)))
    open(os.path.join(scene, "traj.txt"), "w").write("\n".join(lines) + "\n")
    json.dump({"camera": {"w": cam.W, "h": cam.H, "fx": cam.fx, "fy": cam.fy, "cx": cam.cx, "cy": cam.cy, "scale": 6553.5}},
              open(os.path.join(root, "Replica", "cam_params.json"), "w"))
    return scene


def _config(root, scene, save):
    base = os.path.join(ROOT, "tests", "golden", "configs", "replica_base.yaml")
    path = os.path.join(root, "run.yaml")
    # the overrides tests/test_sequence_gpu.py uses at this size; device_list / pcd_densify are ignored / skipped
    open(path, "w").write(f"""parent: "{base}"
source_path: "{scene}"
save_path: "{save}"
save_step: 10
frame_start: 0
frame_step: 0
frame_num: -1
uniform_sample_num: 10200
gaussian_update_iter: 30
stable_confidence_thres: 40.0
unstable_time_window: 24
max_depth: 8.0
keyframe_trans_thes: 0.25
seed: 1
""")
    return path


def _run(argv, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "rtg_slam_amd"] + argv, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_slam_then_metric_from_config(tmp_path):
    scene = _write_dataset(str(tmp_path))
    save = os.path.join(str(tmp_path), "out")
    cfg = _config(str(tmp_path), scene, save)
    out = _run(["slam", "--config", cfg, "--io-workers", "4"], 900)
    assert "device_list" in out and "pcd_densify skipped" in out
    for f in ("config.yaml", "performance.json", "run_report.json", "save_traj/pose_es.npy", "save_traj/pose_gt.npy",
              "save_traj/ate.txt", "eval_metric/slam_eval.csv"):
        assert os.path.isfile(os.path.join(save, f)), f
    frames = sorted(os.listdir(os.path.join(save, "save_model")))
    assert frames == ["frame_0000", "frame_0009", "frame_0019", f"frame_{N:04d}"], frames
    for fr in frames:
        names = os.listdir(os.path.join(save, "save_model", fr))
        # an empty cloud writes no file (as the reference): at frame 0 nothing is stable yet
        assert any(n.startswith("iter_") and n.endswith("_sibr.ply") for n in names), names
    es = np.load(os.path.join(save, "save_traj", "pose_es.npy"))
    gt = np.load(os.path.join(save, "save_traj", "pose_gt.npy"))
    assert es.shape == gt.shape == (N, 4, 4)
    ate = [float(x) for x in open(os.path.join(save, "save_traj", "ate.txt")).read().split()]
    assert len(ate) == N and ate[-1] < 1.0, ate[-1]                        # cm
    perf = json.load(open(os.path.join(save, "performance.json")))
    assert set(perf) == {"tracking", "mapping", "fps"} and perf["fps"] > 0
    rep = json.load(open(os.path.join(save, "run_report.json")))
    assert rep["frames"] == N and rep["ate_rmse_m"] < 0.01
    for k in ("io_wait_s_mean", "decode_ms_per_frame", "io_workers", "wall_fps_including_io"):
        assert rep[k] is not None, k
    assert rep["io_workers"] == 4
    with open(os.path.join(save, "eval_metric", "slam_eval.csv")) as f:
        ev = list(csv.DictReader(f))
    assert len(ev) == 5 and ev[-1]["frame"] == "mean"                     # frames 0, 9, 19, the final row, and the mean
    import yaml
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert merged["uniform_sample_num"] == 10200 and merged["type"] == "Replica" and merged["feature_lr_coef"] == 4.0

    # a non-empty save_path is refused without --overwrite
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "rtg_slam_amd", "slam", "--config", cfg], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and "--overwrite" in r.stdout

    _run(["metric", "--config", cfg], 600)                                # metric.py's default: the stable cloud
    final = os.path.join(save, "save_model", f"frame_{N:04d}")
    csvs = [n for n in os.listdir(save) if n.startswith(f"statis_frame_{N}_iter_")]
    assert len(csvs) == 1, csvs
    with open(os.path.join(save, csvs[0])) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == N + 1 and rows[-1]["frame"] == "mean"

    # the same evaluation in process, on the same model file
    from rtg_slam_amd import __main__ as cli, config, datasets, evaluation
    args = config.load_config(cfg)
    model = cli.filter_models(final, False, [])[0]
    assert model.endswith("_stable.ply"), model
    mapper = cli.load_map(args, DEV, os.path.join(final, model))
    args.frame_num = N
    info = datasets.load_dataset(args)
    res = evaluation.evaluate_sequence(mapper, info.camera(), datasets.FrameSource(info, DEV), poses=es, args=args)
    assert len(res["rows"]) == N
    for row, want in zip(rows[:N], res["rows"]):
        assert int(row["frame"]) == want["frame"]
        for k in ("psnr", "ssim", "depth_loss", "valid_pixel_ratio", "color_l1"):
            a, b = float(row[k]), float(want[k])
            assert abs(a - b) <= 1e-5 * max(abs(b), 1e-12), (k, row["frame"], a, b)
