"""End to end: `python -m rtg_slam_amd slam`, `mesh` and then `metric --mesh --align`, on the Replica-layout dataset of
tests/test_mesh_depth_cli_gpu.py (the synthetic box room, 20 frames, half the Replica size).  So that the answer is known, the
mesh `metric` scores is then replaced by the dataset's GT mesh moved by inverse(pose_t0) and by the inverse of a known small
rigid transform: the registration must find that transform, and the aligned figures must be those of a perfect reconstruction."""
import json
import os

import numpy as np
import pytest

from rtg_slam_amd import io_formats as iof
from tests import mesh_register_reference as ref
from tests.test_mesh_depth_cli_gpu import MESH, N, _cli, _one, _read, _write_config, _write_scene
from tests.test_mesh_register_cpu import BOUND

pytestmark = pytest.mark.gpu
KNOWN = ref.rigid((-0.3, 0.8, 0.5), 0.8, (0.011, -0.007, 0.009))          # 0.8 degrees, 1.6 cm
KEYS = ("transform", "registration", "unaligned", "aligned")
REG_KEYS = ("iterations", "converged", "reason", "inliers", "inlier_share", "rms_plane_before", "rms_plane_after",
            "rms_distance_before", "rms_distance_after", "rank", "rotation_deg", "translation_m", "query_s", "accumulate_s")
PCD_KEYS = ("accuracy", "completion", "P (< 0.03)", "R (< 0.03)", "F1 (< 0.03)")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from rtg_slam_amd import config, datasets
    root = str(tmp_path_factory.mktemp("align_cli"))
    scene, gv, gf = _write_scene(root)
    save = os.path.join(root, "out")
    cfg = _write_config(root, scene, save)
    _cli(["slam", "--config", cfg, "--io-workers", "4"], 900)
    _cli(["mesh", "--config", cfg] + MESH, 600)
    ply = os.path.join(save, "save_model", "mesh_tsdf.ply")
    pose_t0 = np.asarray(datasets.read_pose_t0(config.load_config(cfg)), dtype=np.float64)
    gv, gf = iof.load_mesh_ply(os.path.join(scene, "room0.ply"))
    moved = ref.apply(np.linalg.inv(pose_t0) @ np.linalg.inv(KNOWN), gv)
    iof.save_mesh_ply(ply, moved.astype(np.float32), gf)
    return {"scene": scene, "gv": gv, "gf": gf, "save": save, "cfg": cfg, "ply": ply, "metric": os.path.join(save, "eval_metric"),
            "pose_t0": pose_t0}


def test_metric_align(run):
    import torch
    from rtg_slam_amd import evaluation
    cfg, metric = run["cfg"], run["metric"]
    _cli(["metric", "--config", cfg, "--mesh"], 600)
    statis = _one(run["save"], f"statis_frame_{N}_iter_")
    plain = _read(statis)
    assert not os.path.isdir(metric) or not [n for n in os.listdir(metric) if n.startswith("aligned")]

    out = _cli(["metric", "--config", cfg, "--mesh", "--align"], 600)
    assert _read(statis) == plain                                            # byte for byte what it is without the flag
    path = _one(metric, f"aligned_frame_{N}_iter_")
    got = json.load(open(path))
    assert all(k in got for k in KEYS) and "surface_aligned" not in got and "surface_unaligned" not in got, sorted(got)
    reg = got["registration"]
    assert all(k in reg for k in REG_KEYS), sorted(reg)
    assert all(k in got["aligned"] for k in PCD_KEYS) and list(got["aligned"]) == list(got["unaligned"])
    assert reg["converged"] and reg["rank"] == 6 and reg["query_s"] > 0 and reg["accumulate_s"] > 0 and reg["inlier_share"] > 0.9
    # the transform undoes the known one: what is left moves no GT vertex by more than the CPU test's bound
    T = np.asarray(got["transform"], dtype=np.float64)
    assert T.shape == (4, 4) and np.allclose(np.asarray(got["transform_total"]), T @ run["pose_t0"], atol=1e-12)
    left = np.linalg.norm(ref.apply(T @ np.linalg.inv(KNOWN), run["gv"]) - run["gv"].astype(np.float64), axis=1).max()
    print("iterations", reg["iterations"], "inliers", reg["inliers"], "rotation", reg["rotation_deg"], "translation", reg["translation_m"])
    print("largest displacement of a GT vertex left after the alignment:", left, "bound", BOUND)
    assert abs(reg["rotation_deg"] - 0.8) < 1e-3
    assert left <= BOUND
    print("accuracy", got["unaligned"]["accuracy"], "->", got["aligned"]["accuracy"])
    assert got["aligned"]["accuracy"] < got["unaligned"]["accuracy"]
    # `unaligned` is eval_pcd of the mesh's samples, as metric --mesh computes it
    mv, mf = iof.load_mesh_ply(run["ply"])
    gt_points, _ = iof.sample_mesh_surface(run["gv"], run["gf"], 1_000_000)
    rec = evaluation.sample_mesh_points(mv, mf, 1_000_000, 0, torch.device("cuda:0"))
    want = evaluation.eval_pcd(rec, gt_points, [0.03], run["pose_t0"], 1_000_000)
    assert got["unaligned"] == want
    assert (f"aligned: rotation {reg['rotation_deg']:.4f} deg, translation {100 * reg['translation_m']:.4f} cm, "
            f"{reg['inlier_share']:.4f} inliers; accuracy {want['accuracy']:.4f} -> {got['aligned']['accuracy']:.4f} cm, completion "
            f"{want['completion']:.4f} -> {got['aligned']['completion']:.4f} cm, F1 {want['F1 (< 0.03)']:.3f} -> "
            f"{got['aligned']['F1 (< 0.03)']:.3f} -> {path}") in out

    # with --surface-distance: the exact surface figures, before and after
    _cli(["metric", "--config", cfg, "--mesh", "--align", "--surface-distance"], 600)
    assert _read(statis) == plain
    both = json.load(open(path))
    sd = json.load(open(_one(metric, f"surface_distance_frame_{N}_iter_")))
    assert all(k in both for k in KEYS + ("surface_unaligned", "surface_aligned"))
    assert both["transform"] == got["transform"] and both["aligned"] == got["aligned"]             # two runs, the same bits
    assert list(both["surface_aligned"]) == list(both["surface_unaligned"])
    for k, w in both["surface_unaligned"].items():
        assert sd[k] == w, k
    print("surface accuracy", both["surface_unaligned"]["accuracy"], "->", both["surface_aligned"]["accuracy"])
    assert both["surface_aligned"]["accuracy"] < both["surface_unaligned"]["accuracy"]
    assert both["surface_aligned"]["completion"] < both["surface_unaligned"]["completion"]


def test_refusals(run):
    cfg = run["cfg"]
    out = _cli(["metric", "--config", cfg, "--mesh", "--align", "--align-max-distance", "0"], 300, expect=2)
    assert "--align-max-distance must be > 0" in out
    out = _cli(["metric", "--config", cfg, "--mesh", "--align", "--align-iterations", "0"], 300, expect=2)
    assert "--align-iterations >= 1" in out
    gt = os.path.join(run["scene"], "room0.ply")
    os.replace(gt, gt + ".away")
    try:
        out = _cli(["metric", "--config", cfg, "--align"], 300, expect=2)
    finally:
        os.replace(gt + ".away", gt)
    assert "--align: there is no GT mesh" in out
