"""End to end: `slam --map-exposure --map-exposure-channels rgb` on a short Replica-layout box room whose frames change white
balance (the writer of tests/test_mesh_cli_gpu.py with a tint per frame), then `metric` without and with --exposure-aware: the two
new files appear with the stated columns and every other file is byte for byte what it is without the flag."""
import csv
import json
import os

import numpy as np
import pytest
from PIL import Image

from rtg_slam_amd import synth
from tests import test_mesh_cli_gpu as mesh_cli

pytestmark = pytest.mark.gpu
N = 8
TINTS = [(1.0, 1.0, 1.0)] + [((1.2, 0.9, 1.05) if k % 2 else (0.85, 1.1, 0.95)) for k in range(1, N)]
COLUMNS = ["frame", "psnr", "psnr_ea", "ssim_ea", "color_l1_ea", "gain_r", "gain_g", "gain_b", "offset_r", "offset_g", "offset_b", "code"]


def _write_dataset(root):
    cam = mesh_cli._half_replica()
    scene = os.path.join(root, "Replica", "room0")
    os.makedirs(os.path.join(scene, "results"))
    lines = []
    for i, p in enumerate(synth.trajectory(N, seed=21)):
        d = synth.box_room_depth(cam, p)
        col = synth.box_room_color(cam, p, d).permute(1, 2, 0).double().numpy() * np.asarray(TINTS[i])
        raw = np.clip(np.round(d[..., 0].double().numpy() * 6553.5), 0, 65535).astype(np.uint16)
        Image.fromarray(raw).save(os.path.join(scene, "results", f"depth{i:06d}.png"))
        Image.fromarray(np.clip(np.round(col * 255), 0, 255).astype(np.uint8)).save(os.path.join(scene, "results", f"frame{i:06d}.jpg"),
                                                                                    quality=95)
        lines.append(" ".join(repr(float(v)) for v in p.numpy().reshape(-1)))
    open(os.path.join(scene, "traj.txt"), "w").write("\n".join(lines) + "\n")
    json.dump({"camera": {"w": cam.W, "h": cam.H, "fx": cam.fx, "fy": cam.fy, "cx": cam.cx, "cy": cam.cy, "scale": 6553.5}},
              open(os.path.join(root, "Replica", "cam_params.json"), "w"))
    return scene


def _files(save):
    out = {}
    for base, _, names in os.walk(save):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, save)] = open(p, "rb").read()
    return out


def test_metric_exposure_aware_adds_two_files_and_changes_no_other(tmp_path):
    import yaml
    scene = _write_dataset(str(tmp_path))
    save = os.path.join(str(tmp_path), "out")
    cfg = mesh_cli._config(str(tmp_path), scene, save)
    out = mesh_cli._run(["slam", "--config", cfg, "--io-workers", "2", "--map-exposure", "--map-exposure-channels", "rgb"], 900)
    assert "map exposure: channels rgb" in out
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert merged["map_exposure"] is True and merged["map_exposure_channels"] == "rgb"
    rep = json.load(open(os.path.join(save, "run_report.json")))["map_exposure"]
    assert rep["channels"] == "rgb" and rep["frames_fitted"] == N - 1 and "alpha_r_mean" in rep

    mesh_cli._run(["metric", "--config", cfg], 600)
    before = _files(save)
    statis = [n for n in before if n.startswith(f"statis_frame_{N}_iter_")]
    assert len(statis) == 1 and not any("exposure" in n for n in before)

    out = mesh_cli._run(["metric", "--config", cfg, "--exposure-aware"], 600)
    after = _files(save)
    new = sorted(set(after) - set(before))
    it = statis[0][len(f"statis_frame_{N}_iter_"):-len(".csv")]
    assert new == sorted([os.path.join("eval_metric", f"exposure_frame_{N}_iter_{it}.csv"), os.path.join("eval_metric", "exposure_report.json")])
    for n in before:
        assert after[n] == before[n], n                                         # statis_frame_*.csv among them
    with open(os.path.join(save, new[0])) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == COLUMNS and len(rows) == N and [int(r["frame"]) for r in rows] == list(range(N))
    with open(os.path.join(save, statis[0])) as f:
        plain = list(csv.DictReader(f))
    for r, p in zip(rows, plain):
        assert r["psnr"] == p["psnr"] and int(r["code"]) == 0
    report = json.load(open(os.path.join(save, "eval_metric", "exposure_report.json")))
    for k in ("psnr", "psnr_ea", "ssim_ea", "color_l1_ea", "gain_r", "offset_b", "frames", "frames_refused", "gates", "device_s"):
        assert k in report, k
    assert report["frames"] == N and report["frames_refused"] == 0 and report["device_s"] > 0
    assert report["gates"]["dst_lo"] == 4 / 255 and report["gates"]["huber"] == 0.05 and report["gates"]["iters"] == 4
    assert report["psnr_ea"] > report["psnr"]                                    # the map is in frame 0's balance, the frames are not
    line = [l for l in out.splitlines() if "exposure-aware: PSNR" in l]
    assert len(line) == 1 and f"over {N} frames, 0 refused" in line[0] and new[0] in line[0]
