"""End to end: `python -m rtg_slam_amd slam`, `mesh --decimate 0.25 --texture` and then `metric --mesh-color`: the CSV, the report,
the saved PNGs, the statis CSV byte for byte against a run without the flag, the flag beside --mesh, --mesh-depth and --cull-gt,
and its refusals, on the Replica-layout dataset of tests/test_mesh_depth_cli_gpu.py (the synthetic box room, 20 frames, half the
Replica size, with a GT mesh; its writer and config, copied; one `slam` and one `mesh` run serve every test)."""
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
from tests import visibility_reference as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20
MESH = ["--voxel", "0.02", "--decimate", "0.25", "--texture"]
COLUMNS = ("mesh_hit_ratio", "mesh_psnr", "mesh_ssim", "mesh_color_l1", "mesh_color_l1_hit")


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
    return scene


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
    """slam, then mesh --voxel 0.02 --decimate 0.25 --texture, then metric without the flag."""
    root = str(tmp_path_factory.mktemp("mesh_color_cli"))
    scene = _write_scene(root)
    save = os.path.join(root, "out")
    cfg = _write_config(root, scene, save)
    _cli(["slam", "--config", cfg, "--io-workers", "4"], 900)
    _cli(["mesh", "--config", cfg] + MESH, 600)
    _cli(["metric", "--config", cfg], 600)
    model, metric = os.path.join(save, "save_model"), os.path.join(save, "eval_metric")
    statis = _one(save, f"statis_frame_{N}_iter_")
    assert not os.path.isdir(metric) or not [n for n in os.listdir(metric) if n.startswith("mesh_color")]
    return {"save": save, "cfg": cfg, "ply": os.path.join(model, "mesh_tsdf.ply"), "obj": os.path.join(model, "mesh_textured.obj"),
            "metric": metric, "statis": statis, "plain": _read(statis)}


def _check_csv(path, suffixes):
    rows = _rows(path)
    keys = [k + s for s in suffixes for k in COLUMNS]
    assert len(rows) == N and list(rows[0]) == ["frame"] + keys and [int(r["frame"]) for r in rows] == list(range(N))
    for r in rows:
        assert all(math.isfinite(float(r[k])) for k in keys), r
        for s in suffixes:
            assert 0 < float(r["mesh_hit_ratio" + s]) <= 1 and float(r["mesh_psnr" + s]) > 0
            assert float(r["mesh_ssim" + s]) <= 1 and float(r["mesh_color_l1_hit" + s]) > 0
    return rows, keys


def test_metric_mesh_color_both(run):
    cfg, metric = run["cfg"], run["metric"]
    out = _cli(["metric", "--config", cfg, "--mesh-color", "both", "--mesh-color-save-every", "2"], 600)
    assert _read(run["statis"]) == run["plain"]                                  # name, keys and values untouched
    assert not [n for n in os.listdir(metric) if n.startswith("mesh_depth")]     # --mesh-depth was not asked for
    path = _one(metric, f"mesh_color_frame_{N}_iter_")
    rows, keys = _check_csv(path, ("", "_tex"))
    rep = json.load(open(os.path.join(metric, "mesh_color_report.json")))
    for k in keys:
        assert abs(rep[k] - np.mean([float(r[k]) for r in rows])) <= 1e-12 * max(1.0, abs(rep[k])), k
    _, _, _, image = iof.load_textured_obj(run["obj"])
    assert rep["frames"] == N and rep["source"] == "both" and rep["atlas_size"] == [image.shape[1], image.shape[0]]
    assert rep["render_s"] > 0 and rep["texture_render_s"] > 0 and rep["saved_every"] == 2
    assert os.path.samefile(rep["mesh"], run["ply"]) and os.path.samefile(rep["textured_mesh"], run["obj"])
    print({k: rep[k] for k in keys})
    assert (f"mesh colour: PSNR {rep['mesh_psnr']:.3f} dB (vertex) / {rep['mesh_psnr_tex']:.3f} dB (texture), hit ratio "
            f"{rep['mesh_hit_ratio']:.4f}, {N} frames -> {path}") in out
    cam = _camera()
    pictures = os.path.join(metric, "mesh_color")
    assert sorted(os.listdir(pictures)) == sorted(f"frame_{i:04d}_{s}.png" for i in range(0, N, 2) for s in ("vertex", "texture"))
    for name in os.listdir(pictures):
        with Image.open(os.path.join(pictures, name)) as im:
            assert im.size == (cam.W, cam.H) and im.mode == "RGB"
            assert np.asarray(im).max() > 0


def test_mesh_color_beside_the_other_flags(run):
    cfg, metric = run["cfg"], run["metric"]
    out = _cli(["metric", "--config", cfg, "--mesh-color", "texture", "--mesh", "--mesh-depth", "--cull-gt"], 900)
    rows, keys = _check_csv(_one(metric, f"mesh_color_frame_{N}_iter_"), ("_tex",))
    rep = json.load(open(os.path.join(metric, "mesh_color_report.json")))
    assert rep["source"] == "texture" and rep["mesh"] is None and rep["render_s"] is None and rep["saved_every"] is None
    assert "(vertex) / " in out and "PSNR - (vertex)" in out
    assert len(_rows(_one(metric, f"mesh_depth_frame_{N}_iter_"))) == N
    assert os.path.isfile(os.path.join(metric, "gt_mesh_culled.ply"))
    both = _cli(["metric", "--config", cfg, "--mesh-color", "vertex", "--mesh-depth"], 600)
    assert _read(run["statis"]) == run["plain"]
    _check_csv(_one(metric, f"mesh_color_frame_{N}_iter_"), ("",))
    assert "/ - (texture)" in both


def test_refusals(run):
    cfg = run["cfg"]
    for argv, words in ((["--mesh-color-save-every", "2"], "needs --mesh-color"),
                        (["--mesh-color", "both", "--mesh-color-save-every", "0"], "K >= 1")):
        assert words in _cli(["metric", "--config", cfg] + argv, 300, expect=2)
    for path, flags in ((run["ply"], ("vertex", "both")), (run["obj"], ("texture", "both"))):
        os.replace(path, path + ".away")
        try:
            for flag in flags:
                out = _cli(["metric", "--config", cfg, "--mesh-color", flag], 300, expect=2)
                assert "does not exist" in out and "rtg_slam_amd mesh --config" in out, out[-500:]
            if path == run["obj"]:
                assert "--texture" in out
        finally:
            os.replace(path + ".away", path)
    v, f = iof.load_mesh_ply(run["ply"])
    os.replace(run["ply"], run["ply"] + ".away")
    try:
        iof.save_mesh_ply(run["ply"], v, f)                                      # the same mesh without colours
        out = _cli(["metric", "--config", cfg, "--mesh-color", "vertex"], 300, expect=2)
        assert "no vertex colours" in out and "rtg_slam_amd mesh --config" in out
    finally:
        os.replace(run["ply"] + ".away", run["ply"])


def test_mesh_color_at_half_the_resolution(run):
    """The last test: --resolution-scale rewrites the statis CSV at another picture size."""
    cfg, metric = run["cfg"], run["metric"]
    _cli(["metric", "--config", cfg, "--resolution-scale", "2", "--mesh-color", "both", "--mesh-color-save-every", "10"], 600)
    _check_csv(_one(metric, f"mesh_color_frame_{N}_iter_"), ("", "_tex"))
    cam = _camera()
    for name in ("frame_0000_vertex.png", "frame_0010_texture.png"):
        with Image.open(os.path.join(metric, "mesh_color", name)) as im:
            assert im.size == (cam.W // 2, cam.H // 2)
