"""`python -m rtg_slam_amd slam --rgbd-refine` on the on-disk synthetic dataset of tests/test_run_config_gpu.py: the option
reaches config.yaml and run_report.json only when it is given, and a weight of 0 is refused."""
import json
import os
import subprocess
import sys

import pytest
import yaml

from tests.test_run_config_gpu import ROOT, _config, _write_dataset

pytestmark = pytest.mark.gpu
FRAMES = 5


def _slam(argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "rtg_slam_amd", "slam"] + argv, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=600)


def test_flag_reaches_config_and_report_only_when_given(tmp_path):
    scene = _write_dataset(str(tmp_path))
    keys = ("rgbd_refine", "rgbd_refine_photo_weight", "rgbd_refine_huber")

    save = os.path.join(str(tmp_path), "refined")
    cfg = _config(str(tmp_path), scene, save)
    r = _slam(["--config", cfg, "--frames", str(FRAMES), "--rgbd-refine", "--rgbd-refine-photo-weight", "0.5"])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "rgbd refine: on (photo weight 0.5, huber 0.05)" in r.stdout
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert merged["rgbd_refine"] is True and merged["rgbd_refine_photo_weight"] == 0.5
    assert "rgbd_refine_huber" not in merged                                  # not given: not written
    rep = json.load(open(os.path.join(save, "run_report.json")))
    assert rep["frames"] == FRAMES
    rr = rep["rgbd_refine"]
    assert rr["frames"] == FRAMES - 1 and rr["photo_weight"] == 0.5 and rr["huber"] == 0.05
    assert 0 < rr["iterations_mean"] <= 9 and rr["photometric_inliers_mean"] > 1000 and rr["ms_mean"] > 0

    save = os.path.join(str(tmp_path), "plain")
    cfg = _config(str(tmp_path), scene, save)
    r = _slam(["--config", cfg, "--frames", str(FRAMES)])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "rgbd refine" not in r.stdout
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert not any(k in merged for k in keys)
    assert "rgbd_refine" not in json.load(open(os.path.join(save, "run_report.json")))

    save = os.path.join(str(tmp_path), "refused")
    cfg = _config(str(tmp_path), scene, save)
    r = _slam(["--config", cfg, "--rgbd-refine", "--rgbd-refine-photo-weight", "0"])
    assert r.returncode == 2, r.stdout[-2000:] + r.stderr[-2000:]
    assert "must be positive" in r.stdout
    assert not os.path.exists(save)
