"""End to end: `python -m rtg_slam_amd mesh` with --min-component-faces, --simplify and --normals, `metric --mesh` on the cleaned
file, and `mesh` without the options against mesh_from_map's default output, on the small Replica-layout run of
tests/test_mesh_cli_gpu.py (its dataset writer and config, copied; one `slam` run serves both tests)."""
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
# what mesh_report.json held before the clean-up options existed
PARENT_KEYS = {"voxel", "trunc", "dims", "bounds", "depth_source", "every", "frames_fused", "V", "F", "render_s", "integrate_s",
               "extract_s", "total_s", "write_s", "model"}
CLEANUP_KEYS = {"V_raw", "F_raw", "components", "components_removed", "faces_removed", "vertices_removed", "simplify_cell", "normals",
                "cleanup_s"}


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


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One `slam` run on the synthetic dataset -> (scene directory, config path, save_path)."""
    root = str(tmp_path_factory.mktemp("cleanup_cli"))
    scene = _write_dataset(root)
    save = os.path.join(root, "out")
    cfg = _config(root, scene, save)
    _run(["slam", "--config", cfg, "--io-workers", "4"], 900)
    return scene, cfg, save


def _ply_header(path):
    with open(path, "rb") as f:
        head = f.read(2048)
    return head[:head.index(b"end_header")].decode("ascii").split("\n")


def test_mesh_with_the_cleanup_options(run):
    scene, cfg, save = run
    model_dir = os.path.join(save, "save_model")
    ply, rep_path = os.path.join(model_dir, "mesh_tsdf.ply"), os.path.join(model_dir, "mesh_report.json")

    # a cell that is not larger than the voxel: refused, with the reason
    out = _run(["mesh", "--config", cfg, "--voxel", "0.02", "--simplify", "0.02"], 300, expect=2)
    assert "must be larger than the voxel" in out

    out = _run(["mesh", "--config", cfg, "--voxel", "0.02", "--min-component-faces", "200", "--simplify", "0.05", "--normals"], 600)
    assert ply in out and "clean-up:" in out
    head = _ply_header(ply)
    props = [l.split()[-1] for l in head if l.startswith("property") and "list" not in l]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"], head
    rep = json.load(open(rep_path))
    assert set(rep) == PARENT_KEYS | CLEANUP_KEYS, sorted(set(rep) ^ (PARENT_KEYS | CLEANUP_KEYS))
    print({k: rep[k] for k in sorted(CLEANUP_KEYS | {"V", "F"})})
    assert 0 < rep["F"] <= rep["F_raw"] and 0 < rep["V"] <= rep["V_raw"]
    assert rep["normals"] is True and abs(rep["simplify_cell"] - 0.05) < 1e-9
    assert rep["components_removed"] <= rep["components"] and rep["faces_removed"] <= rep["F_raw"]
    assert f"{rep['V_raw']} vertices, {rep['F_raw']} faces raw -> {rep['V']} vertices, {rep['F']} faces" in out
    assert f"{rep['components_removed']} of {rep['components']} components removed" in out
    v, f, c = iof.load_mesh_ply(ply, with_colors=True)
    assert v.shape == (rep["V"], 3) and f.shape == (rep["F"], 3) and f.min() >= 0 and f.max() < rep["V"]
    assert c is not None and c.min() >= 0 and c.max() <= 1 and np.isfinite(v).all()
    lo, hi = np.asarray(rep["bounds"][0]), np.asarray(rep["bounds"][1])
    assert (v >= lo - 1e-4).all() and (v <= hi + 1e-4).all()

    # metric --mesh scores the cleaned file against a GT mesh (the plain box: 12 triangles)
    hx, hy, hz = 2.5, 1.5, 3.0
    bv = np.array([[sx * hx, sy * hy, sz * hz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    bf = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)
    iof.save_mesh_ply(os.path.join(scene, "room0.ply"), bv, bf)
    out = _run(["metric", "--config", cfg, "--mesh"], 600)
    assert f"geometry eval mesh: {ply}" in out
    csvs = [n for n in os.listdir(save) if n.startswith(f"statis_frame_{N}_iter_")]
    assert len(csvs) == 1, csvs
    with open(os.path.join(save, csvs[0])) as fh:
        last = list(csv.DictReader(fh))[N - 1]
    assert math.isfinite(float(last["accuracy"])) and math.isfinite(float(last["completion"]))
    print({k: last[k] for k in last if k.startswith(("accuracy", "completion", "P ", "R ", "F1"))})
    os.remove(os.path.join(scene, "room0.ply"))


def test_mesh_without_the_options_is_unchanged(run, tmp_path):
    """The file `mesh` writes equals save_mesh_ply of mesh_from_map's default output, and the report has the old keys."""
    import torch
    from rtg_slam_amd import __main__ as cli, config, datasets, meshing
    scene, cfg, save = run
    model_dir = os.path.join(save, "save_model")
    _run(["mesh", "--config", cfg, "--voxel", "0.02"], 600)
    rep = json.load(open(os.path.join(model_dir, "mesh_report.json")))
    assert set(rep) == PARENT_KEYS, sorted(set(rep) ^ PARENT_KEYS)
    written = open(os.path.join(model_dir, "mesh_tsdf.ply"), "rb").read()
    assert b"property float nx" not in written[:1024]

    # the command's own steps, in this process
    opts = cli.build_parser().parse_args(["mesh", "--config", cfg, "--voxel", "0.02"])
    args = config.load_config(cfg)
    cli._apply_resolution_scale(args, opts)
    device = torch.device("cuda", 0)
    model_base, check_frame, select_ply, test_iter = cli.select_model(args, opts)
    mapper = cli.load_map(args, device, select_ply)
    mapper.time, mapper.iter = int(check_frame.split("_")[1]), int(test_iter)
    poses = None
    if not args.use_gt_pose:
        poses = np.load(os.path.join(args.save_path, "save_traj", "pose_es.npy")).reshape(-1, 4, 4)[int(args.frame_start):]
    args.frame_num = int(check_frame.split("_")[-1])
    info = datasets.load_dataset(args)
    source = datasets.FrameSource(info, device, io_workers=None)
    result = meshing.mesh_from_map(mapper, info.camera(), poses, source, voxel=0.02, trunc=4.0 * 0.02, args=args, device=device)
    assert len(result) == 4
    vertices, faces, colors, report = result
    assert set(report) == PARENT_KEYS - {"total_s", "write_s", "model"}
    assert report["V"] == rep["V"] and report["F"] == rep["F"]
    mine = str(tmp_path / "mine.ply")
    iof.save_mesh_ply(mine, vertices, faces, colors)
    assert open(mine, "rb").read() == written
