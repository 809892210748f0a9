"""`python -m rtg_slam_amd slam --loop-closure --loop-closure-candidates ...` on the on-disk synthetic dataset of
tests/test_run_config_gpu.py: the appearance flags reach config.yaml and the report only when given, and are refused without
--loop-closure or with a bad value before anything is written.  (That a run without them writes no loop_closure key at all
is tests/test_loop_closure_cli_gpu.py's.)"""
import json
import os

import pytest
import yaml

from tests.test_loop_closure_cli_gpu import FRAMES, _slam
from tests.test_run_config_gpu import _config, _write_dataset

pytestmark = pytest.mark.gpu


def test_appearance_flags_reach_config_and_report_only_when_given(tmp_path):
    scene = _write_dataset(str(tmp_path))
    save = os.path.join(str(tmp_path), "closed")
    cfg = _config(str(tmp_path), scene, save)
    r = _slam(["--config", cfg, "--frames", str(FRAMES), "--loop-closure", "--loop-closure-min-gap", "2",
               "--loop-closure-candidates", "both", "--loop-closure-thumb-width", "16", "--loop-closure-min-score", "0.95"])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert merged["loop_closure"] is True and merged["loop_closure_candidates"] == "both"
    assert merged["loop_closure_thumb_width"] == 16 and merged["loop_closure_min_score"] == 0.95
    assert "loop_closure_max_shift" not in merged and "loop_closure_max_depth_rel" not in merged      # not given: not written
    lc = json.load(open(os.path.join(save, "run_report.json")))["loop_closure"]
    app = lc["appearance"]
    assert app["mode"] == "both" and app["thumbnail"][0] == 16 and app["max_shift"] == 4 and app["min_score"] == 0.95
    assert {"describe", "scores"} <= set(lc["seconds"]) and all("source" in c for c in lc["candidates"])
    assert "candidates" not in lc["options"] and "thumb_width" not in lc["options"]

    save = os.path.join(str(tmp_path), "refused")
    cfg = _config(str(tmp_path), scene, save)
    for argv, said in ((["--loop-closure-candidates", "appearance"], "needs --loop-closure"),
                       (["--loop-closure", "--loop-closure-candidates", "orb"], "invalid choice"),
                       (["--loop-closure", "--loop-closure-thumb-width", "8", "--loop-closure-max-shift", "4"], "must stay below")):
        r = _slam(["--config", cfg] + argv)
        assert r.returncode == 2, r.stdout[-2000:] + r.stderr[-2000:]
        assert said in r.stdout + r.stderr
        assert not os.path.exists(save)
