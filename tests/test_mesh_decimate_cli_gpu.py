"""End to end: `python -m rtg_slam_amd mesh` with --decimate and --decimate-max-error, alone and with the other clean-up
options, its refusals, and `mesh` without them against mesh_from_map's default output, on the small Replica-layout run of
tests/test_mesh_cleanup_cli_gpu.py (its dataset writer and config, copied; one `slam` run serves every test)."""
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
# what mesh_report.json holds without any option, with the clean-up options, and what --decimate adds
PARENT_KEYS = {"voxel", "trunc", "dims", "bounds", "depth_source", "every", "frames_fused", "V", "F", "render_s", "integrate_s",
               "extract_s", "total_s", "write_s", "model"}
CLEANUP_KEYS = {"V_raw", "F_raw", "simplify_cell", "normals", "cleanup_s"}
REMOVAL_KEYS = {"components", "components_removed", "faces_removed", "vertices_removed"}
DECIMATE_KEYS = {"decimate", "decimate_max_error", "F_before_decimate", "decimate_rounds", "decimate_collapses",
                 "decimate_target_reached", "decimate_s"}


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
    root = str(tmp_path_factory.mktemp("decimate_cli"))
    scene = _write_dataset(root)
    save = os.path.join(root, "out")
    cfg = _config(root, scene, save)
    _run(["slam", "--config", cfg, "--io-workers", "4"], 900)
    return scene, cfg, save


def _outputs(save):
    model_dir = os.path.join(save, "save_model")
    return os.path.join(model_dir, "mesh_tsdf.ply"), os.path.join(model_dir, "mesh_report.json")


def test_mesh_decimate(run):
    scene, cfg, save = run
    ply, rep_path = _outputs(save)
    out = _run(["mesh", "--config", cfg, "--voxel", "0.02", "--decimate", "0.25"], 600)
    assert ply in out and "decimation:" in out
    rep = json.load(open(rep_path))
    assert set(rep) == PARENT_KEYS | CLEANUP_KEYS | DECIMATE_KEYS, sorted(set(rep) ^ (PARENT_KEYS | CLEANUP_KEYS | DECIMATE_KEYS))
    print({k: rep[k] for k in sorted(DECIMATE_KEYS | {"V", "F", "V_raw", "F_raw", "cleanup_s"})})
    target = int(0.25 * rep["F_before_decimate"])
    assert rep["F_before_decimate"] == rep["F_raw"] and rep["decimate"] == 0.25 and rep["decimate_max_error"] is None
    assert rep["decimate_target_reached"] is True and target - 1 <= rep["F"] <= target
    assert rep["F_raw"] - rep["F"] == 2 * rep["decimate_collapses"] and 0 < rep["decimate_rounds"] < 1000
    assert 0 < rep["decimate_s"] <= rep["cleanup_s"]
    assert f"{rep['F_before_decimate']} faces -> {rep['F']} faces" in out
    assert f"{rep['decimate_collapses']} collapses in {rep['decimate_rounds']} rounds, target reached" in out
    v, f, c = iof.load_mesh_ply(ply, with_colors=True)
    assert v.shape == (rep["V"], 3) and f.shape == (rep["F"], 3) and f.min() >= 0 and f.max() < rep["V"]
    assert c is not None and c.min() >= 0 and c.max() <= 1 and np.isfinite(v).all()
    assert len(np.unique(f)) == rep["V"]                                          # no vertex is left unused
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
    lo, hi = np.asarray(rep["bounds"][0]), np.asarray(rep["bounds"][1])
    assert (v >= lo - 1e-4).all() and (v <= hi + 1e-4).all()

    # with an error bound that nothing passes it stops where it started, and says so
    out = _run(["mesh", "--config", cfg, "--voxel", "0.02", "--decimate", "0.25", "--decimate-max-error", "1e-12"], 600)
    bounded = json.load(open(rep_path))
    assert bounded["decimate_max_error"] == 1e-12 and bounded["F"] > target and bounded["decimate_target_reached"] is False
    assert "target NOT reached" in out and "error <= 1e-12 m" in out


def test_mesh_decimate_with_the_other_options(run):
    scene, cfg, save = run
    ply, rep_path = _outputs(save)
    out = _run(["mesh", "--config", cfg, "--voxel", "0.02", "--decimate", "0.25", "--normals", "--min-component-faces", "50"], 600)
    assert "clean-up:" in out and "decimation:" in out
    rep = json.load(open(rep_path))
    assert set(rep) == PARENT_KEYS | CLEANUP_KEYS | REMOVAL_KEYS | DECIMATE_KEYS
    assert rep["normals"] is True and rep["F_before_decimate"] == rep["F_raw"] - rep["faces_removed"]
    target = int(0.25 * rep["F_before_decimate"])
    assert rep["decimate_target_reached"] is True and target - 1 <= rep["F"] <= target
    with open(ply, "rb") as fh:
        head = fh.read(2048)
    head = head[:head.index(b"end_header")].decode("ascii").split("\n")
    props = [l.split()[-1] for l in head if l.startswith("property") and "list" not in l]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"], head
    v, f, c = iof.load_mesh_ply(ply, with_colors=True)
    assert v.shape == (rep["V"], 3) and f.shape == (rep["F"], 3)
    assert len(np.unique(f)) == rep["V"] and np.isfinite(v).all()


def test_refusals(run):
    scene, cfg, save = run
    for argv, words in ((["--decimate", "1"], "--decimate 1"),
                        (["--decimate", "0.5", "--decimate-max-error", "0"], "--decimate-max-error must be > 0"),
                        (["--decimate-max-error", "0.01"], "needs --decimate")):
        out = _run(["mesh", "--config", cfg, "--voxel", "0.02"] + argv, 300, expect=2)
        assert words in out, (argv, out[-500:])


def test_mesh_without_the_options_is_unchanged(run, tmp_path):
    """The file `mesh` writes equals save_mesh_ply of mesh_from_map's default output, with the clean-up options of before on
    or off, and the report has the keys of before."""
    import torch
    from rtg_slam_amd import __main__ as cli, config, datasets, meshing
    scene, cfg, save = run
    ply, rep_path = _outputs(save)

    def in_this_process(**options):
        opts = cli.build_parser().parse_args(["mesh", "--config", cfg, "--voxel", "0.02"])
        assert opts.decimate == 0.0 and opts.decimate_max_error is None
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
        return meshing.mesh_from_map(mapper, info.camera(), poses, source, voxel=0.02, trunc=4.0 * 0.02, args=args, device=device,
                                     **options)

    _run(["mesh", "--config", cfg, "--voxel", "0.02"], 600)
    rep = json.load(open(rep_path))
    assert set(rep) == PARENT_KEYS, sorted(set(rep) ^ PARENT_KEYS)
    written = open(ply, "rb").read()
    vertices, faces, colors, report = in_this_process()
    assert set(report) == PARENT_KEYS - {"total_s", "write_s", "model"}
    mine = str(tmp_path / "mine.ply")
    iof.save_mesh_ply(mine, vertices, faces, colors)
    assert open(mine, "rb").read() == written

    _run(["mesh", "--config", cfg, "--voxel", "0.02", "--min-component-faces", "200", "--simplify", "0.05", "--normals"], 600)
    rep = json.load(open(rep_path))
    assert set(rep) == PARENT_KEYS | CLEANUP_KEYS | REMOVAL_KEYS
    written = open(ply, "rb").read()
    vertices, faces, colors, report, normals = in_this_process(min_component_faces=200, simplify_cell=0.05, normals=True)
    assert set(report) == (PARENT_KEYS | CLEANUP_KEYS | REMOVAL_KEYS) - {"total_s", "write_s", "model"}
    iof.save_mesh_ply(mine, vertices, faces, colors, normals)
    assert open(mine, "rb").read() == written
