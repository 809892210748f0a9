"""End to end: `python -m rtg_slam_amd slam`, then `metric` without and with --cull-gt, on a Replica-layout dataset written to
disk from the synthetic box room (20 frames, half the Replica size) whose GT mesh is the flat room plus a cube annex behind
its wall that no frame can see."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from rtg_slam_amd import io_formats as iof, synth
from tests import visibility_reference as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20
GEOMETRY = ("accuracy", "completion", "P (", "R (", "F1 (")


def _camera():
    c = synth.REPLICA
    return synth.CameraSpec(c.H // 2, c.W // 2, c.fx / 2, c.fy / 2, (c.cx + 0.5) / 2 - 0.5, (c.cy + 0.5) / 2 - 0.5)


def _write_scene(root):
    """results/depthNNNNNN.png + frameNNNNNN.jpg, traj.txt, ../cam_params.json and the GT mesh room0.ply."""
    cam = _camera()
    scene = os.path.join(root, "Replica", "room0")
    results = os.path.join(scene, "results")
    os.makedirs(results)
    with open(os.path.join(scene, "traj.txt"), "w") as traj:
        for i, pose in enumerate(synth.trajectory(N, seed=21)):
            depth = synth.box_room_depth(cam, pose)
            color = synth.box_room_color(cam, pose, depth)
            png = np.clip(np.round(depth[..., 0].double().numpy() * 6553.5), 0, 65535).astype(np.uint16)
            jpg = np.clip(np.round(color.permute(1, 2, 0).double().numpy() * 255), 0, 255).astype(np.uint8)
            Image.fromarray(png).save(os.path.join(results, f"depth{i:06d}.png"))
            Image.fromarray(jpg).save(os.path.join(results, f"frame{i:06d}.jpg"), quality=95)
            traj.write(" ".join(repr(float(x)) for x in pose.numpy().reshape(-1)) + "\n")
    with open(os.path.join(root, "Replica", "cam_params.json"), "w") as f:
        json.dump({"camera": {"w": cam.W, "h": cam.H, "fx": cam.fx, "fy": cam.fy, "cx": cam.cx, "cy": cam.cy, "scale": 6553.5}}, f)
    gv, gf, _ = vr.room_and_annex()
    iof.save_mesh_ply(os.path.join(scene, "room0.ply"), gv, gf)
    return scene, gv, gf


def _write_config(root, scene, save):
    path = os.path.join(root, "run.yaml")
    base = os.path.join(ROOT, "tests", "golden", "configs", "replica_base.yaml")
    settings = {"parent": f'"{base}"', "source_path": f'"{scene}"', "save_path": f'"{save}"', "save_step": 10, "frame_start": 0,
                "frame_step": 0, "frame_num": -1, "uniform_sample_num": 10200, "gaussian_update_iter": 30,
                "stable_confidence_thres": 40.0, "unstable_time_window": 24, "max_depth": 8.0, "keyframe_trans_thes": 0.25,
                "seed": 1}
    with open(path, "w") as f:
        f.write("".join(f"{k}: {v}\n" for k, v in settings.items()))
    return path


def _cli(argv, timeout, expect=0):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "rtg_slam_amd"] + argv, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == expect, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def _csv_rows(save):
    names = [n for n in os.listdir(save) if n.startswith(f"statis_frame_{N}_iter_")]
    assert len(names) == 1, names
    with open(os.path.join(save, names[0])) as f:
        return list(csv.DictReader(f))


def test_metric_cull_gt_from_config(tmp_path):
    root = str(tmp_path)
    scene, gv, gf = _write_scene(root)
    save = os.path.join(root, "out")
    cfg = _write_config(root, scene, save)
    _cli(["slam", "--config", cfg, "--io-workers", "4"], 900)
    ply = os.path.join(save, "eval_metric", "gt_mesh_culled.ply")
    rep_path = os.path.join(save, "eval_metric", "gt_cull_report.json")

    out = _cli(["metric", "--config", cfg], 600)
    assert "culled" not in out and not os.path.exists(ply) and not os.path.exists(rep_path)
    plain = _csv_rows(save)

    assert "--cull-min-views" in _cli(["metric", "--config", cfg, "--cull-gt", "--cull-min-views", "0"], 300, expect=2)
    assert not os.path.exists(ply)

    # the walls carry a 5 cm relief that the flat GT lacks: a tolerance of 0.1
    out = _cli(["metric", "--config", cfg, "--cull-gt", "--cull-tolerance", "0.1"], 600)
    culled = _csv_rows(save)
    assert os.path.isfile(ply) and os.path.isfile(rep_path)
    rep = json.load(open(rep_path))
    cv, cf = iof.load_mesh_ply(ply)
    assert rep["F"] == len(gf) and rep["V"] == len(gv) and rep["frames"] == N
    assert rep["F_kept"] == len(cf) and rep["V_kept"] == len(cv) and 0 < rep["F_kept"] < rep["F"]
    assert abs(rep["tolerance"] - 0.1) < 1e-7 and rep["min_views"] == 1 and rep["keep"] == "all" and rep["seconds"] > 0
    assert rep["gt_mesh"] == os.path.join(scene, "room0.ply")
    assert f"geometry eval gt: culled {rep['F_kept']} of {rep['F']} faces over {N} frames -> {ply}" in out
    assert not (cv[:, 0] > 2.6).any()                                   # nothing of the annex
    assert cf.min() >= 0 and cf.max() < len(cv)
    gt_rows = {r.tobytes() for r in np.ascontiguousarray(gv, dtype="<f4")}
    assert all(r.tobytes() in gt_rows for r in np.ascontiguousarray(cv, dtype="<f4"))

    a, b = plain[N - 1], culled[N - 1]
    print({k: (a[k], b[k]) for k in a if k.startswith(GEOMETRY)})
    assert float(b["completion"]) < float(a["completion"])              # cm: the unseen room and the annex left the GT
    assert float(b["R (< 0.03)"]) > float(a["R (< 0.03)"])
    assert len(plain) == len(culled) == N + 1 and list(a) == list(b)          # the frames, then the mean row
    pictures = [k for k in a if not k.startswith(GEOMETRY)]
    assert "psnr" in pictures and "depth_loss" in pictures
    for ra, rb in zip(plain, culled):
        assert [ra[k] for k in pictures] == [rb[k] for k in pictures]
