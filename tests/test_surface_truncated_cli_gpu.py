"""End to end: `metric --mesh --surface-distance --surface-max-distance D` on the run of tests/test_surface_distance_cli_gpu.py
(the Replica-layout box room of tests/test_mesh_depth_cli_gpu.py: slam over 20 frames, then mesh).  The flag adds three keys and
a log line; without it the files are what they were."""
import json
import os

import pytest

from tests.test_mesh_depth_cli_gpu import MESH, N, _cli, _one, _read, _write_config, _write_scene

pytestmark = pytest.mark.gpu
NEW = ("max_distance", "beyond_acc", "beyond_comp")
FRACTIONS = ("P (< 0.03)", "R (< 0.03)", "F1 (< 0.03)")
SURFACE = ["--mesh", "--surface-distance"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("surface_truncated_cli"))
    scene, gv, gf = _write_scene(root)
    save = os.path.join(root, "out")
    cfg = _write_config(root, scene, save)
    _cli(["slam", "--config", cfg, "--io-workers", "4"], 900)
    _cli(["mesh", "--config", cfg] + MESH, 600)
    return {"save": save, "cfg": cfg, "metric": os.path.join(save, "eval_metric")}


def _timeless(text):
    """The JSON text of a surface_distance file with its clock readings zeroed: everything else is deterministic."""
    d = json.loads(text)
    d["seconds"] = 0
    for side in ("distance_gt", "distance_rec"):
        d[side]["build_s"] = d[side]["query_s"] = 0
    return json.dumps(d, indent=1)


def test_surface_max_distance(run):
    cfg, metric = run["cfg"], run["metric"]
    _cli(["metric", "--config", cfg] + SURFACE, 600)
    path = _one(metric, f"surface_distance_frame_{N}_iter_")
    statis = _one(run["save"], f"statis_frame_{N}_iter_")
    before, before_statis = _read(path).decode(), _read(statis)
    plain = json.loads(before)
    assert not set(NEW) & set(plain)

    out = _cli(["metric", "--config", cfg] + SURFACE + ["--surface-max-distance", "0.05", "--align"], 900)
    got = json.load(open(path))
    assert [k for k in got if k not in NEW] == list(plain) and all(k in got for k in NEW), sorted(got)   # its keys, in order, and three
    assert got["max_distance"] == 0.05 and 0 <= got["beyond_acc"] <= 1_000_000 and 0 < got["beyond_comp"] <= 1_000_000   # the annex
    for k in FRACTIONS:
        assert got[k] == plain[k], k
    assert got["accuracy"] <= plain["accuracy"] and got["completion"] < plain["completion"]
    assert got["normal_samples_comp"] == 1_000_000 - got["beyond_comp"]
    assert f"surface distance truncated at 0.05 m: {got['beyond_acc']} / {got['beyond_comp']} samples beyond" in out
    assert _read(statis) == before_statis
    al = json.load(open(_one(metric, f"aligned_frame_{N}_iter_")))
    assert all(k in al["surface_aligned"] for k in NEW) and list(al["surface_aligned"]) == list(al["surface_unaligned"])
    assert al["surface_aligned"]["max_distance"] == 0.05 and al["surface_unaligned"]["beyond_comp"] == got["beyond_comp"]

    out = _cli(["metric", "--config", cfg] + SURFACE, 600)
    assert "surface distance truncated at" not in out
    after = _read(path).decode()
    assert _timeless(after) == _timeless(before)                           # byte for byte but for the clock readings
    assert _read(statis) == before_statis
    assert list(json.loads(after)) == list(plain)


def test_refusals(run):
    cfg = run["cfg"]
    out = _cli(["metric", "--config", cfg, "--mesh", "--surface-max-distance", "0.05"], 300, expect=2)
    assert "--surface-max-distance needs --surface-distance" in out
    for bad in ("0.03", "nan", "inf"):                                     # not above the threshold, not finite
        out = _cli(["metric", "--config", cfg] + SURFACE + ["--surface-max-distance", bad], 300, expect=2)
        assert "--surface-max-distance must be" in out
