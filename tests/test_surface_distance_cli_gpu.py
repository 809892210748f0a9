"""End to end: `python -m rtg_slam_amd slam`, `mesh` and then `metric --mesh --surface-distance`, on the Replica-layout dataset
of tests/test_mesh_depth_cli_gpu.py (the synthetic box room, 20 frames, half the Replica size; its GT mesh is the flat room plus
a cube annex behind its wall).  The written figures are recomputed from the written PLY, the GT mesh and
evaluation.eval_mesh_surface, which tests/test_mesh_distance_gpu.py holds to the numpy definition."""
import json
import os

import pytest

from rtg_slam_amd import io_formats as iof
from tests.test_mesh_depth_cli_gpu import MESH, N, _cli, _one, _read, _write_config, _write_scene

pytestmark = pytest.mark.gpu
KEYS = ("accuracy", "completion", "P (< 0.03)", "R (< 0.03)", "F1 (< 0.03)", "normal_consistency_acc", "normal_consistency_comp",
        "normal_consistency", "normal_samples_acc", "normal_samples_comp", "V", "F", "V_gt", "F_gt", "distance_gt", "distance_rec",
        "seconds")
REPORT_KEYS = ("cell", "dims", "entries", "bytes", "large_faces", "build_s", "query_s")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("surface_distance_cli"))
    scene, gv, gf = _write_scene(root)
    save = os.path.join(root, "out")
    cfg = _write_config(root, scene, save)
    _cli(["slam", "--config", cfg, "--io-workers", "4"], 900)
    _cli(["mesh", "--config", cfg] + MESH, 600)
    return {"scene": scene, "gv": gv, "gf": gf, "save": save, "cfg": cfg, "ply": os.path.join(save, "save_model", "mesh_tsdf.ply"),
            "metric": os.path.join(save, "eval_metric")}


def test_metric_surface_distance(run):
    from rtg_slam_amd import config, datasets, evaluation
    cfg, metric = run["cfg"], run["metric"]
    _cli(["metric", "--config", cfg, "--mesh"], 600)
    statis = _one(run["save"], f"statis_frame_{N}_iter_")
    plain = _read(statis)
    assert not os.path.isdir(metric) or not [n for n in os.listdir(metric) if n.startswith("surface_distance")]

    out = _cli(["metric", "--config", cfg, "--mesh", "--surface-distance"], 600)
    assert _read(statis) == plain                                            # byte for byte what it is without the flag
    path = _one(metric, f"surface_distance_frame_{N}_iter_")
    got = json.load(open(path))
    assert all(k in got for k in KEYS), sorted(got)
    for side in ("distance_gt", "distance_rec"):
        assert all(k in got[side] for k in REPORT_KEYS) and got[side]["entries"] > 0 and got[side]["query_s"] > 0
    mv, mf = iof.load_mesh_ply(run["ply"])
    assert (got["V"], got["F"], got["V_gt"], got["F_gt"]) == (len(mv), len(mf), len(run["gv"]), len(run["gf"]))
    assert got["seconds"] > 0 and got["gt_culled"] is False
    gv, gf = iof.load_mesh_ply(os.path.join(run["scene"], "room0.ply"))
    want = evaluation.eval_mesh_surface(mv, mf, gv, gf, dist_thres=[0.03], transform=datasets.read_pose_t0(config.load_config(cfg)),
                                        sample_nums=1_000_000, device="cuda:0")
    for k, w in want.items():
        assert got[k] == w, (k, got[k], w)                                   # the same kernels, the same order: the same bits
    assert 0 < got["accuracy"] < 10 and 0 < got["completion"] and 0 < got["normal_consistency"] <= 1
    assert (f"surface distance: accuracy {got['accuracy']:.4f} cm, completion {got['completion']:.4f} cm, F1 {got['F1 (< 0.03)']:.3f}, "
            f"normal consistency {got['normal_consistency']:.4f} -> {path}") in out

    # against the culled GT: the annex no frame saw no longer counts against the completion
    out = _cli(["metric", "--config", cfg, "--mesh", "--surface-distance", "--cull-gt"], 600)
    culled = json.load(open(path))
    print("completion", got["completion"], "culled", culled["completion"])
    assert culled["gt_culled"] is True and culled["F_gt"] < got["F_gt"] and culled["completion"] < got["completion"]


def test_refusals(run):
    cfg = run["cfg"]
    out = _cli(["metric", "--config", cfg, "--surface-distance"], 300, expect=2)
    assert "--surface-distance needs --mesh" in out
    gt = os.path.join(run["scene"], "room0.ply")
    os.replace(gt, gt + ".away")
    try:
        out = _cli(["metric", "--config", cfg, "--mesh", "--surface-distance"], 300, expect=2)
    finally:
        os.replace(gt + ".away", gt)
    assert "--surface-distance: there is no GT mesh" in out
    os.replace(run["ply"], run["ply"] + ".away")
    try:
        out = _cli(["metric", "--config", cfg, "--mesh", "--surface-distance"], 300, expect=2)
    finally:
        os.replace(run["ply"] + ".away", run["ply"])
    assert "does not exist" in out and "rtg_slam_amd mesh --config" in out
