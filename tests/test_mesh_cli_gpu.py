"""End to end: `python -m rtg_slam_amd slam`, then `mesh` (rendered and sensor depth) and `metric` with and without --mesh, on a
Replica-layout dataset written to disk from the synthetic box room (the writer of tests/test_run_config_gpu.py, copied)."""
import csv
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from rtg_slam_amd import io_formats as iof, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _run(argv, timeout, expect=0):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "rtg_slam_amd"] + argv, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == expect, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _check_mesh(model_dir, source, frames):
    ply, rep_path = os.path.join(model_dir, "mesh_tsdf.ply"), os.path.join(model_dir, "mesh_report.json")
    assert os.path.isfile(ply) and os.path.isfile(rep_path)
    rep = json.load(open(rep_path))
    for k in ("voxel", "trunc", "dims", "bounds", "frames_fused", "V", "F", "render_s", "integrate_s", "extract_s", "write_s"):
        assert k in rep, k
    assert rep["depth_source"] == source and rep["frames_fused"] == frames
    assert abs(rep["voxel"] - 0.02) < 1e-7 and abs(rep["trunc"] - 0.08) < 1e-6 and len(rep["dims"]) == 3
    v, f, c = iof.load_mesh_ply(ply, with_colors=True)
    assert v.shape == (rep["V"], 3) and f.shape == (rep["F"], 3) and rep["V"] > 0 and rep["F"] > 0
    assert f.min() >= 0 and f.max() < rep["V"]
    assert c is not None and c.min() >= 0 and c.max() <= 1 and np.isfinite(v).all()
    lo, hi = np.asarray(rep["bounds"][0]), np.asarray(rep["bounds"][1])
    assert (v >= lo - 1e-4).all() and (v <= hi + 1e-4).all()
    return rep


def _rows(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def test_mesh_and_metric_mesh_from_config(tmp_path):
    scene = _write_dataset(str(tmp_path))
    save = os.path.join(str(tmp_path), "out")
    cfg = _config(str(tmp_path), scene, save)
    _run(["slam", "--config", cfg, "--io-workers", "4"], 900)
    model_dir = os.path.join(save, "save_model")

    _run(["metric", "--config", cfg], 600)
    csvs = [n for n in os.listdir(save) if n.startswith(f"statis_frame_{N}_iter_")]
    assert len(csvs) == 1, csvs
    before = open(os.path.join(save, csvs[0]), "rb").read()

    # --mesh without a mesh: a clear message, nothing evaluated
    out = _run(["metric", "--config", cfg, "--mesh"], 300, expect=2)
    assert "mesh_tsdf.ply does not exist" in out

    out = _run(["mesh", "--config", cfg, "--voxel", "0.02"], 600)
    assert os.path.join(model_dir, "mesh_tsdf.ply") in out
    rendered = _check_mesh(model_dir, "render", N)

    # metric without --mesh: the mesh file changes nothing
    _run(["metric", "--config", cfg], 600)
    assert open(os.path.join(save, csvs[0]), "rb").read() == before

    # with --mesh and a GT mesh (the plain box: 12 triangles) the reconstruction metrics come from the mesh
    hx, hy, hz = 2.5, 1.5, 3.0
    bv = np.array([[sx * hx, sy * hy, sz * hz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    bf = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)
    iof.save_mesh_ply(os.path.join(scene, "room0.ply"), bv, bf)
    out = _run(["metric", "--config", cfg, "--mesh"], 600)
    assert f"geometry eval mesh: {os.path.join(model_dir, 'mesh_tsdf.ply')}" in out
    rows = _rows(os.path.join(save, csvs[0]))
    last = rows[N - 1]
    print({k: last[k] for k in last if k.startswith(("accuracy", "completion", "P ", "R ", "F1"))})
    assert math.isfinite(float(last["accuracy"])) and math.isfinite(float(last["completion"]))
    assert float(last["accuracy"]) < 10.0                  # cm: the mesh lies on the walls (their relief is up to ~4 cm)

    out = _run(["mesh", "--config", cfg, "--voxel", "0.02", "--depth-source", "sensor", "--every", "2"], 600)
    sensor = _check_mesh(model_dir, "sensor", N // 2)
    assert sensor["dims"] == rendered["dims"]               # the same map, the same default bounds
    print("rendered:", rendered)
    print("sensor:", sensor)
