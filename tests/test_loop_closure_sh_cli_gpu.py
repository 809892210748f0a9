"""`python -m rtg_slam_amd slam --loop-closure --loop-closure-rotate-sh` on the on-disk synthetic dataset of
tests/test_run_config_gpu.py: the key reaches config.yaml and the log only when given, and without --loop-closure it is refused
before anything is written."""
import json
import os

import pytest
import yaml

from tests.test_loop_closure_cli_gpu import FRAMES, _slam
from tests.test_run_config_gpu import _config, _write_dataset

pytestmark = pytest.mark.gpu


def test_flag_reaches_config_and_log_only_when_given(tmp_path):
    scene = _write_dataset(str(tmp_path))

    save = os.path.join(str(tmp_path), "turned")
    cfg = _config(str(tmp_path), scene, save)
    r = _slam(["--config", cfg, "--frames", str(FRAMES), "--loop-closure", "--loop-closure-rotate-sh", "--loop-closure-min-gap", "2"])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    on = [line for line in r.stdout.splitlines() if "loop closure: on" in line]
    assert len(on) == 1 and "higher SH bands turned" in on[0]
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert merged["loop_closure"] is True and merged["loop_closure_rotate_sh"] is True
    lc = json.load(open(os.path.join(save, "run_report.json")))["loop_closure"]
    assert lc["edges"] == 0 and not lc["changed"] and "sh_rotated" not in lc    # five frames: nothing closed, nothing turned
    assert "rotate_sh" not in lc["options"]

    save = os.path.join(str(tmp_path), "plain")
    cfg = _config(str(tmp_path), scene, save)
    r = _slam(["--config", cfg, "--frames", str(FRAMES), "--loop-closure", "--loop-closure-min-gap", "2"])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    on = [line for line in r.stdout.splitlines() if "loop closure: on" in line]
    assert len(on) == 1 and "SH" not in on[0]
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert merged["loop_closure"] is True and "loop_closure_rotate_sh" not in merged
    assert "sh_rotated" not in json.load(open(os.path.join(save, "run_report.json")))["loop_closure"]

    save = os.path.join(str(tmp_path), "refused")
    cfg = _config(str(tmp_path), scene, save)
    r = _slam(["--config", cfg, "--loop-closure-rotate-sh"])
    assert r.returncode == 2, r.stdout[-2000:] + r.stderr[-2000:]
    assert "needs --loop-closure" in r.stdout + r.stderr
    assert not os.path.exists(save)
