"""End to end: `python -m rtg_slam_amd slam`, `mesh` and then `metric --mesh-depth`, `metric --cull-gt --cull-depth mesh` and
`mesh --cull-unseen`, on the Replica-layout dataset of tests/test_cull_gt_cli_gpu.py (the synthetic box room, 20 frames, half
the Replica size; its GT mesh is the flat room plus a cube annex behind its wall that no frame can see).  The figures of
--mesh-depth are recomputed here from the written PLY, the saved poses, the decoded frames and tests/mesh_render_reference.py."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from rtg_slam_amd import io_formats as iof, synth
from tests import mesh_render_reference as rr
from tests import visibility_reference as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20
MESH = ["--voxel", "0.1", "--depth-source", "sensor"]
NEW_MESH_KEYS = ("cull_unseen", "F_unseen_removed", "V_unseen_removed", "cull_render_s")


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


def _one(directory, prefix):
    names = [n for n in os.listdir(directory) if n.startswith(prefix)]
    assert len(names) == 1, names
    return os.path.join(directory, names[0])


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _rows(path):
    with open(path) as f:
        return list(csv.DictReader(f))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """slam, then mesh --voxel 0.1 --depth-source sensor: a mesh small enough for the numpy reference."""
    root = str(tmp_path_factory.mktemp("mesh_depth_cli"))
    scene, gv, gf = _write_scene(root)
    save = os.path.join(root, "out")
    cfg = _write_config(root, scene, save)
    _cli(["slam", "--config", cfg, "--io-workers", "4"], 900)
    out = _cli(["mesh", "--config", cfg] + MESH, 600)
    assert "cull unseen" not in out
    model = os.path.join(save, "save_model")
    return {"root": root, "scene": scene, "gv": gv, "gf": gf, "save": save, "cfg": cfg, "ply": os.path.join(model, "mesh_tsdf.ply"),
            "report": os.path.join(model, "mesh_report.json"), "metric": os.path.join(save, "eval_metric")}


def _recompute(run, frames):
    """{frame: (ratio, l1, ratio_gt, l1_gt)} from the PLY, pose_es.npy, the decoded frames and the numpy definition."""
    import torch
    from rtg_slam_amd import config, datasets
    args = config.load_config(run["cfg"])
    args.frame_num = N
    info = datasets.load_dataset(args)
    cam = info.camera()
    K = (cam.fx, cam.fy, cam.cx, cam.cy)
    poses = None
    if not args.use_gt_pose:
        poses = np.load(os.path.join(run["save"], "save_traj", "pose_es.npy")).reshape(-1, 4, 4)[int(args.frame_start):]
    pose_t0 = datasets.read_pose_t0(args)
    mv, mf = iof.load_mesh_ply(run["ply"])
    want = {}
    for i, (depth, _, gt_c2w) in enumerate(datasets.FrameSource(info, torch.device("cuda:0"), io_workers=2)):
        if i not in frames:
            continue
        sensor = depth.reshape(cam.H, cam.W).cpu().numpy()
        c2w = np.asarray(poses[i] if poses is not None else gt_c2w, dtype=np.float64)
        mesh_depth, _ = rr.render(mv, mf, K, cam.H, cam.W, c2w)
        gt_depth, _ = rr.render(run["gv"], run["gf"], K, cam.H, cam.W, pose_t0 @ np.asarray(gt_c2w, dtype=np.float64))
        want[i] = (rr.depth_metrics(mesh_depth, sensor, args.min_depth, args.max_depth)
                   + rr.depth_metrics(mesh_depth, gt_depth, args.min_depth, args.max_depth))
    return want


def test_metric_mesh_depth(run):
    cfg, metric = run["cfg"], run["metric"]
    _cli(["metric", "--config", cfg], 600)
    statis = _one(run["save"], f"statis_frame_{N}_iter_")
    plain = _read(statis)
    assert not [n for n in os.listdir(metric) if n.startswith("mesh_depth")]

    out = _cli(["metric", "--config", cfg, "--mesh-depth"], 600)
    assert _read(statis) == plain                                            # name, keys and values untouched
    path = _one(metric, f"mesh_depth_frame_{N}_iter_")
    rows = _rows(path)
    keys = ["mesh_valid_ratio", "mesh_depth_l1", "mesh_valid_ratio_gt", "mesh_depth_l1_gt"]
    assert len(rows) == N and list(rows[0]) == ["frame"] + keys and [int(r["frame"]) for r in rows] == list(range(N))
    want = _recompute(run, (0, N - 1))
    for i, w in want.items():
        got = [float(rows[i][k]) for k in keys]
        print(i, got, w)
        assert got[0] == w[0] and got[2] == w[2]
        assert abs(got[1] - w[1]) <= 1e-6 * w[1] and abs(got[3] - w[3]) <= 1e-6 * w[3]
        assert 0 < w[0] <= 1.0 and 0 < w[2] <= 1.0 and w[1] > 0 and w[3] > 0
    rep = json.load(open(os.path.join(metric, "mesh_depth_report.json")))
    for k in keys:
        assert abs(rep[k] - np.mean([float(r[k]) for r in rows])) <= 1e-12
    assert rep["frames"] == N and abs(rep["near"] - 0.05) < 1e-8 and rep["render_s"] > 0 and rep["gt_render_s"] > 0
    assert f"mesh depth: L1 {100 * rep['mesh_depth_l1']:.3f} cm over {rep['mesh_valid_ratio']:.4f} of the pixels, {N} frames -> {path}" in out
    run["mesh_depth_csv"] = _read(path)


def test_cull_depth_mesh(run):
    cfg, metric = run["cfg"], run["metric"]
    assert "--cull-gt" in _cli(["metric", "--config", cfg, "--cull-depth", "mesh"], 300, expect=2)
    rep_path, ply = os.path.join(metric, "gt_cull_report.json"), os.path.join(metric, "gt_mesh_culled.ply")
    _cli(["metric", "--config", cfg, "--cull-gt"], 600)
    sensor = json.load(open(rep_path))
    assert "depth" not in sensor
    _cli(["metric", "--config", cfg, "--cull-gt", "--cull-depth", "mesh", "--mesh-depth"], 600)
    rep = json.load(open(rep_path))
    cv, cf = iof.load_mesh_ply(ply)
    assert rep["depth"] == "mesh" and rep["F_kept"] == len(cf) and rep["V_kept"] == len(cv) and rep["frames"] == N
    assert not (cv[:, 0] > 2.6).any()                                        # nothing of the annex
    # the flat GT wall is never behind its own render; the sensor's relief of up to 5 cm hides part of it at 0.03
    print("F_kept", sensor["F_kept"], rep["F_kept"], "of", rep["F"])
    assert 0 < sensor["F_kept"] <= rep["F_kept"] < rep["F"]
    if "mesh_depth_csv" in run:                                              # --mesh-depth does not depend on the cull
        assert _read(_one(metric, f"mesh_depth_frame_{N}_iter_")) == run["mesh_depth_csv"]


def test_mesh_cull_unseen(run):
    cfg = run["cfg"]
    plain_ply, plain_rep = _read(run["ply"]), json.load(open(run["report"]))
    assert not set(NEW_MESH_KEYS) & set(plain_rep) and "F_raw" not in plain_rep
    out = _cli(["mesh", "--config", cfg, "--cull-unseen-tolerance", "0.1"] + MESH, 300, expect=2)
    assert "--cull-unseen" in out and _read(run["ply"]) == plain_ply
    try:
        out = _cli(["mesh", "--config", cfg, "--cull-unseen"] + MESH, 600)
        rep = json.load(open(run["report"]))
        v, f = iof.load_mesh_ply(run["ply"])
        assert all(k in rep for k in NEW_MESH_KEYS)
        assert rep["F"] + rep["F_unseen_removed"] == rep["F_raw"] == plain_rep["F"]
        assert rep["V"] + rep["V_unseen_removed"] == rep["V_raw"] == plain_rep["V"]
        assert (len(v), len(f)) == (rep["V"], rep["F"]) and 0 < rep["F"] <= rep["F_raw"]
        assert abs(rep["cull_unseen"] - 0.1) < 1e-7 and rep["cull_render_s"] > 0           # the default: the voxel
        assert f"cull unseen: {rep['F_unseen_removed']} of {rep['F_raw']} faces" in out
    finally:
        _cli(["mesh", "--config", cfg] + MESH, 600)                           # and without the flag: what it wrote before
    again = json.load(open(run["report"]))
    timing = lambda r: {k: v for k, v in r.items() if not k.endswith("_s")}
    assert _read(run["ply"]) == plain_ply and list(again) == list(plain_rep) and timing(again) == timing(plain_rep)


def test_mesh_depth_without_the_mesh(run):
    os.replace(run["ply"], run["ply"] + ".away")
    try:
        out = _cli(["metric", "--config", run["cfg"], "--mesh-depth"], 300, expect=2)
    finally:
        os.replace(run["ply"] + ".away", run["ply"])
    assert "does not exist" in out and "rtg_slam_amd mesh --config" in out
