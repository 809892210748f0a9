"""bench.py's multi-rank launcher path on the one-GPU lease: `python bench.py --gpus 2 --mode X` spawns its two ranks
itself (torch.distributed.run, 127.0.0.1), both share the GPU over gloo (RTGS_DIST_BACKEND=gloo: RCCL refuses two ranks
on one device), every multi-GPU form of the map step runs, rank 0 prints the contract's JSON line.  On the driver's
8-GPU node the same code runs one rank per GPU over RCCL (backend nccl) - this test keeps the launcher, the world-size /
backend assertions and the three forms from rotting in between (BASELINE configs[4]).  The scaling legs,
the roofline and configs[4] are in the line with --full only."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["sparse", "sharded", "tileband", "auto"])
def test_two_ranks_through_the_launcher(mode):
    env = dict(os.environ, RTGS_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--prewarm", "4",
           "--full", "--repeats", "1", "--gaussians", "60000", "--no-cpu-baseline", "--no-surface", "--no-schedule",
           "--config5-gaussians", "80000"] + ([] if mode == "auto" else ["--mode", mode])
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 0 and d["value"] > 0 and d["steps"] == 3
    if mode == "auto":                                  # what the driver's N > 1 runs get: ONE stream, split into tile bands
        mode = "tileband"
    assert d["config"]["mode"] == mode and d["scaling"] == ("strong" if mode == "tileband" else "weak")
    assert d["metric"] == "hot_path_units_per_sec" and d["unit"] == "units/s"
    assert d["roofline"]["frac"] > 0
    if mode != "sharded":
        assert d["strong_scaling_one_view"]["n_gpus"] == 2
    # BASELINE configs[4] rides in every line: sharded, 10 iterations, the four-way split of SURVEY.md 8d
    c5 = d["config5"]
    assert c5["n_gpus"] == 2 and c5["mode"] == "sharded" and c5["iterations"] == 10 and c5["ms_per_iteration"] > 0
    assert set(c5["split_ms"]) == {"render_fwd_and_loss", "render_bwd", "collective", "adam"}
    assert c5["split_ms"]["render_fwd_and_loss"] > 0 and c5["split_ms"]["render_bwd"] > 0 and c5["split_ms"]["adam"] > 0
    assert c5["split_ms"]["collective"] > 0                     # two ranks: the exchange exists
    if mode == "tileband":
        w = d["weak_scaling_one_view_per_rank"]
        assert w["n_gpus"] == 2 and w["views_per_sec"] > 0
    else:
        assert d["weak_scaling_one_view_per_rank"] is None


@pytest.mark.parametrize("gpus", [1, 2])
def test_plain_run_prints_the_headline_and_dumps_the_last_step(gpus, tmp_path):
    """Without --full a run times exactly --steps units and prints the headline fields only; --dump-outputs writes what
    the last timed unit computed (float32 / float64 .npy, at most 64 MB).  Two ranks: rank 0 writes, after the collective
    flush of the row exchange."""
    import numpy as np
    env = dict(os.environ, RTGS_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "7", "--warmup", "1",
           "--prewarm", "4", "--gaussians", "60000", "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["n_gpus"] == gpus and d["full"] is False and d["dtype"] == "f32"
    assert d["metric"] == "hot_path_units_per_sec" and d["unit"] == "units/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) / d["value"] < 0.01
    assert "roofline" not in d and "repeats" not in d and "slam_sequence" not in d
    files = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(files) == {"icp_result", "map_loss", "map_losses", "map_xyz_sample", "map_shs_sample", "map_raw8_sample",
                          "map_sample_rows"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["icp_result"].shape == (20,) and np.array_equal(files["icp_result"][12:16], [0, 0, 0, 1])
    assert files["map_xyz_sample"].shape == (60000, 3) and files["map_shs_sample"].shape == (60000, 48)
    assert np.isfinite(files["map_losses"]).all() and files["map_losses"][0] == files["map_loss"]
