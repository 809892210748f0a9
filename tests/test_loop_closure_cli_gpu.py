"""`python -m rtg_slam_amd slam --loop-closure` on the on-disk synthetic dataset of tests/test_run_config_gpu.py: both trajectories
and the report key are written only when the option is given, and a bad value is refused before anything is written."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from tests.test_run_config_gpu import ROOT, _config, _write_dataset

pytestmark = pytest.mark.gpu
FRAMES = 5
BEFORE = os.path.join("save_traj", "pose_es_before_loop_closure.npy")


def _slam(argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "rtg_slam_amd", "slam"] + argv, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=600)


def test_flag_reaches_config_report_and_trajectories_only_when_given(tmp_path):
    scene = _write_dataset(str(tmp_path))

    save = os.path.join(str(tmp_path), "closed")
    cfg = _config(str(tmp_path), scene, save)
    r = _slam(["--config", cfg, "--frames", str(FRAMES), "--loop-closure", "--loop-closure-min-gap", "2",
               "--loop-closure-loop-weights", "4", "9"])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "loop closure: on" in r.stdout and "loop closure: 0 edges of" in r.stdout
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert merged["loop_closure"] is True and merged["loop_closure_min_gap"] == 2 and merged["loop_closure_loop_weights"] == [4.0, 9.0]
    assert "loop_closure_max_trans" not in merged                              # not given: not written
    rep = json.load(open(os.path.join(save, "run_report.json")))
    lc = rep["loop_closure"]
    assert rep["frames"] == FRAMES and lc["frames"] == FRAMES and lc["keyframes"] >= 1 and lc["edges"] == 0 and not lc["changed"]
    assert lc["options"]["min_gap"] == 2 and lc["options"]["loop_weights"] == [4.0, 9.0] and lc["options"]["max_trans"] == 0.5
    assert lc["ate_rmse_m"] == lc["ate_rmse_m_before"] == rep["ate_rmse_m"] and "total" in lc["seconds"]
    es = np.load(os.path.join(save, "save_traj", "pose_es.npy"))
    before = np.load(os.path.join(save, BEFORE))
    assert es.shape == (FRAMES, 4, 4) and np.array_equal(es, before)           # nothing was accepted: nothing moved

    save = os.path.join(str(tmp_path), "plain")
    cfg = _config(str(tmp_path), scene, save)
    r = _slam(["--config", cfg, "--frames", str(FRAMES)])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "loop closure" not in r.stdout
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert not any(k.startswith("loop_closure") for k in merged)
    assert "loop_closure" not in json.load(open(os.path.join(save, "run_report.json")))
    assert os.path.exists(os.path.join(save, "save_traj", "pose_es.npy")) and not os.path.exists(os.path.join(save, BEFORE))

    save = os.path.join(str(tmp_path), "refused")
    cfg = _config(str(tmp_path), scene, save)
    for argv, said in ((["--loop-closure", "--loop-closure-min-gap", "0"], "must be >= 1"),
                       (["--loop-closure", "--loop-closure-max-rms", "-1"], "must not be negative"),
                       (["--loop-closure-max-trans", "0.3"], "needs --loop-closure"),
                       (["--loop-closure", "--loop-closure-max-trans", "near"], "invalid float value")):
        r = _slam(["--config", cfg] + argv)
        assert r.returncode == 2, r.stdout[-2000:] + r.stderr[-2000:]
        assert said in r.stdout + r.stderr
        assert not os.path.exists(save)
