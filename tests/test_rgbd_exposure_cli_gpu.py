"""`python -m rtg_slam_amd slam --rgbd-refine-target / --rgbd-refine-exposure` on the on-disk synthetic dataset of
tests/test_run_config_gpu.py: the options reach config.yaml, the log and run_report.json only when they are given, and need
--rgbd-refine."""
import json
import os
import subprocess
import sys

import pytest
import yaml

from tests.test_run_config_gpu import ROOT, _config, _write_dataset

pytestmark = pytest.mark.gpu
FRAMES = 5
FIRST_LINE = "rgbd refine: on (photo weight 0.25, huber 0.05)"
NEW_KEYS = ("rgbd_refine_target", "rgbd_refine_exposure")
NEW_REPORT_KEYS = ("target", "exposure", "alpha_mean", "beta_mean", "alpha_min", "alpha_max")


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("rgbd_exposure_cli"))
    return root, _write_dataset(root)


def _slam(argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "rtg_slam_amd", "slam"] + argv, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=600)


def test_flags_reach_config_log_and_report(dataset):
    root, scene = dataset
    save = os.path.join(root, "both")
    cfg = _config(root, scene, save)
    r = _slam(["--config", cfg, "--frames", str(FRAMES), "--rgbd-refine", "--rgbd-refine-target", "model", "--rgbd-refine-exposure"])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert FIRST_LINE in r.stdout
    assert "rgbd refine: target model, exposure on" in r.stdout
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert merged["rgbd_refine"] is True and merged["rgbd_refine_target"] == "model" and merged["rgbd_refine_exposure"] is True
    rep = json.load(open(os.path.join(save, "run_report.json")))
    rr = rep["rgbd_refine"]
    assert rep["frames"] == FRAMES and rr["frames"] == FRAMES - 1
    assert rr["target"] == "model" and rr["exposure"] is True
    # whatever the solve finds lies inside the range the loop accepts
    assert 0.25 <= rr["alpha_min"] <= rr["alpha_mean"] <= rr["alpha_max"] <= 4.0 and abs(rr["beta_mean"]) <= 0.5
    print("exposure over the run:", {k: rr[k] for k in NEW_REPORT_KEYS})
    assert 0 < rr["iterations_mean"] <= 9 and rr["photometric_inliers_mean"] > 1000


def test_without_the_flags_nothing_is_added(dataset):
    root, scene = dataset
    save = os.path.join(root, "alone")
    cfg = _config(root, scene, save)
    r = _slam(["--config", cfg, "--frames", str(FRAMES), "--rgbd-refine"])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert FIRST_LINE in r.stdout and r.stdout.count("rgbd refine:") == 1
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert merged["rgbd_refine"] is True and not any(k in merged for k in NEW_KEYS)
    rr = json.load(open(os.path.join(save, "run_report.json")))["rgbd_refine"]
    assert not any(k in rr for k in NEW_REPORT_KEYS)


@pytest.mark.parametrize("flags", [["--rgbd-refine-target", "model"], ["--rgbd-refine-exposure"]])
def test_flags_need_rgbd_refine(dataset, flags):
    root, scene = dataset
    save = os.path.join(root, "refused")
    cfg = _config(root, scene, save)
    r = _slam(["--config", cfg, "--frames", str(FRAMES)] + flags)
    assert r.returncode == 2, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"{flags[0]} needs --rgbd-refine" in r.stdout
    assert not os.path.exists(save)
