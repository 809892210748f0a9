"""End to end: `python -m rtg_slam_amd mesh --texture`: the three files it writes, what load_textured_obj reads back, the report's
keys, mesh_tsdf.ply byte for byte against the same command without the flag, and its refusals, on the small Replica-layout run
of tests/test_mesh_cli_gpu.py (its dataset writer and config, copied; one `slam` run serves every test)."""
import json
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
# what mesh_report.json holds without any option, with the clean-up options, what --decimate adds and what --texture adds
PARENT_KEYS = {"voxel", "trunc", "dims", "bounds", "depth_source", "every", "frames_fused", "V", "F", "render_s", "integrate_s",
               "extract_s", "total_s", "write_s", "model"}
CLEANUP_KEYS = {"V_raw", "F_raw", "simplify_cell", "normals", "cleanup_s"}
REMOVAL_KEYS = {"components", "components_removed", "faces_removed", "vertices_removed"}
DECIMATE_KEYS = {"decimate", "decimate_max_error", "F_before_decimate", "decimate_rounds", "decimate_collapses",
                 "decimate_target_reached", "decimate_s"}
TEXTURE_KEYS = {"texture_texel", "texture_size", "texture_fill", "texture_seen_share", "texture_views", "texture_faces_capped",
                "texture_s"}
TEXTURE_FILES = ("mesh_textured.obj", "mesh_textured.mtl", "mesh_texture.png")


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
    return r.stdout + r.stderr


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One `slam` run on the synthetic dataset -> (scene directory, config path, save_path)."""
    root = str(tmp_path_factory.mktemp("texture_cli"))
    scene = _write_dataset(root)
    save = os.path.join(root, "out")
    cfg = _config(root, scene, save)
    _run(["slam", "--config", cfg, "--io-workers", "4"], 900)
    return scene, cfg, save



def test_mesh_texture(run):
    scene, cfg, save = run
    model_dir = os.path.join(save, "save_model")
    ply, rep_path = os.path.join(model_dir, "mesh_tsdf.ply"), os.path.join(model_dir, "mesh_report.json")
    base = ["mesh", "--config", cfg, "--voxel", "0.02", "--decimate", "0.25"]

    # without the flag: no texture file, no texture key
    out = _run(base, 600)
    assert "texture:" not in out
    for name in TEXTURE_FILES:
        assert not os.path.exists(os.path.join(model_dir, name)), name
    plain = json.load(open(rep_path))
    assert set(plain) == PARENT_KEYS | CLEANUP_KEYS | DECIMATE_KEYS, sorted(set(plain) ^ (PARENT_KEYS | CLEANUP_KEYS | DECIMATE_KEYS))
    plain_ply = open(ply, "rb").read()

    out = _run(base + ["--texture"], 600)
    for name in TEXTURE_FILES:
        assert os.path.isfile(os.path.join(model_dir, name)), name
    rep = json.load(open(rep_path))
    want = PARENT_KEYS | CLEANUP_KEYS | DECIMATE_KEYS | TEXTURE_KEYS
    assert set(rep) == want, sorted(set(rep) ^ want)
    print({k: rep[k] for k in sorted(TEXTURE_KEYS | {"V", "F"})})
    assert open(ply, "rb").read() == plain_ply, "mesh_tsdf.ply does not depend on --texture"
    assert rep["F"] == plain["F"] and rep["V"] == plain["V"]
    assert abs(rep["texture_texel"] - 0.02) < 1e-9 and rep["texture_views"] == N and rep["texture_s"] > 0
    assert 0 < rep["texture_seen_share"] <= 1 and 0 < rep["texture_fill"] <= 1 and rep["texture_faces_capped"] >= 0
    wt, ht = rep["texture_size"]
    assert wt in (ht, 2 * ht) and wt & (wt - 1) == 0
    obj = os.path.join(model_dir, "mesh_textured.obj")
    assert f"texture: {wt} x {ht}, " in out and f"seen by {N} views -> {obj}" in out
    v, f, uv, image = iof.load_textured_obj(obj)
    assert f.shape == (rep["F"], 3) and v.shape == (rep["V"], 3) and uv.shape == (rep["F"], 3, 2)
    assert uv.min() >= 0 and uv.max() <= 1 and image.shape == (ht, wt, 3) and image.dtype == np.uint8
    pv, pf = iof.load_mesh_ply(ply)
    assert np.array_equal(v, pv.astype(np.float32)) and np.array_equal(f, pf)
    assert "map_Kd mesh_texture.png" in open(os.path.join(model_dir, "mesh_textured.mtl")).read()
    assert image.reshape(-1, 3).max(0).min() > 0                                  # something was painted in every channel

    # a coarser texel and a lower cap
    out = _run(base + ["--texture", "--texture-texel", "0.04", "--texture-max-level", "3"], 600)
    coarse = json.load(open(rep_path))
    assert abs(coarse["texture_texel"] - 0.04) < 1e-9 and coarse["texture_size"][0] <= wt
    assert open(ply, "rb").read() == plain_ply


def test_refusals(run):
    scene, cfg, save = run
    for argv, words in ((["--texture", "--texture-texel", "0"], "--texture-texel 0"),
                        (["--texture", "--texture-max-level", "7"], "--texture-max-level 7"),
                        (["--texture-texel", "0"], "need --texture"),
                        (["--texture", "--texture-texel", "1e-6"], "smallest texel that fits")):
        out = _run(["mesh", "--config", cfg, "--voxel", "0.02"] + argv, 300, expect=2)
        assert words in out, (argv, out[-500:])
