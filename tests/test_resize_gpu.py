"""The resized ingest (rtgs_ingest_rgbd_resized) against the installed Pillow followed by the reference's float chain:
torch.equal on depth and colour.  Then the streaming source with a resized DatasetInfo, and `slam --resolution-scale 2` /
`metric` end to end on a full-size dataset."""
import csv
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from rtg_slam_amd import datasets as ds, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
SCALES = (6553.5, 5000.0, 1000.0)


def _expected(raw, col, scale, crop, out_size):
    """loadCam on the CPU: readCameras' float32 depth and crop, PIL resize (BILINEAR colour, NEAREST depth), PILtoTorch's
    / 255 in torch; then map_preprocess's * 255 on the device."""
    d = np.asarray(raw, dtype=np.float32) / scale
    c = np.array(col)
    if crop > 0:
        d = d[crop:-crop, crop:-crop]
        c = c[crop:-crop, crop:-crop, :]
    c = np.array(Image.fromarray(np.ascontiguousarray(c)).resize(out_size, Image.BILINEAR))
    d = np.array(Image.fromarray(np.ascontiguousarray(d)).resize(out_size, Image.NEAREST))
    d_t = torch.from_numpy(d) / 255.0
    c_t = (torch.from_numpy(c) / 255.0).permute(2, 0, 1)[:3]
    return (d_t.to(DEV) * 255).unsqueeze(-1), c_t.contiguous().to(DEV)


def _run(raw, col, scale, crop, out_size, tables=None):
    return ds.ingest(torch.from_numpy(raw.view(np.int16)).to(DEV), torch.from_numpy(col).to(DEV), scale, crop,
                     out_size=out_size, tables=tables)


def _frame(rng, W, H, channels, crop):
    """Random raw frame of (W + 2 crop) x (H + 2 crop); where it fits, a block holding every u16 value."""
    Hd, Wd = H + 2 * crop, W + 2 * crop
    raw = rng.integers(0, 65536, size=(Hd, Wd), dtype=np.uint16)
    if H >= 256 and W >= 256:
        raw[crop:crop + 256, crop:crop + 256] = rng.permutation(65536).astype(np.uint16).reshape(256, 256)
    col = rng.integers(0, 256, size=(Hd, Wd, channels), dtype=np.uint8)
    return raw, col


# cropped (W, H) -> (Wo, Ho): the reference's scales 2 and 4 on Replica, TUM at 2, a non-integer ratio with odd sizes (no
# vector-store path: Wo = 401), one axis unchanged each way, enlarging, the 1184 x 664 frame a crop of 8 leaves of 1200 x 680
SIZE_PAIRS = [((1200, 680), (600, 340)), ((1200, 680), (300, 170)), ((640, 480), (320, 240)), ((601, 337), (401, 225)),
              ((601, 337), (400, 225)), ((320, 200), (320, 100)), ((320, 200), (160, 200)), ((100, 60), (250, 171)),
              ((1184, 664), (592, 332)), ((37, 23), (5, 3))]


@pytest.mark.parametrize("crop", [0, 8])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("in_size, out_size", SIZE_PAIRS)
def test_resized_ingest_equals_pillow(in_size, out_size, channels, crop):
    (W, H), (Wo, Ho) = in_size, out_size
    rng = np.random.default_rng(W * 131 + Ho * 7 + channels + crop)
    raw, col = _frame(rng, W, H, channels, crop)
    tables = ds.resize_tables(in_size, out_size).to(DEV)
    for k, scale in enumerate(SCALES):
        d, c = _run(raw, col, scale, crop, out_size, tables if k else None)        # with and without prepared tables
        torch.cuda.synchronize()
        de, ce = _expected(raw, col, scale, crop, out_size)
        assert d.shape == (Ho, Wo, 1) and c.shape == (3, Ho, Wo) and d.dtype == c.dtype == torch.float32
        assert torch.equal(d, de), (scale, int((d != de).sum()))
        assert torch.equal(c, ce), (scale, int((c != ce).sum()), float((c - ce).abs().max()) * 255)


def test_every_u8_and_u16_value_occurs():
    """The inputs of the full-frame case above hold every u8 colour value and every u16 depth value inside the crop."""
    for channels in (3, 4):
        for crop in (0, 8):
            rng = np.random.default_rng(1200 * 131 + 340 * 7 + channels + crop)
            raw, col = _frame(rng, 1200, 680, channels, crop)
            inner = (slice(crop, crop + 680), slice(crop, crop + 1200))
            assert np.unique(raw[inner]).size == 65536
            for k in range(channels):
                assert np.unique(col[inner][..., k]).size == 256


def test_saturated_and_zero_frames():
    for value in (0, 255):
        for channels in (3, 4):
            col = np.full((340, 600, channels), value, dtype=np.uint8)
            raw = np.full((340, 600), 65535 if value else 0, dtype=np.uint16)
            for out_size in ((300, 170), (401, 227), (900, 510)):
                d, c = _run(raw, col, 6553.5, 0, out_size)
                de, ce = _expected(raw, col, 6553.5, 0, out_size)
                assert torch.equal(d, de) and torch.equal(c, ce)
                assert float(c.min()) == float(c.max()) == value / 255.0


def test_rgba_alpha_round_trip():
    rng = np.random.default_rng(9)
    col = rng.integers(0, 256, size=(96, 128, 4), dtype=np.uint8)
    col[:32, :, 3] = 0
    col[32:64, :, 3] = 255
    col[64:, :, 3] = np.arange(128, dtype=np.uint8)[None, :] * 2
    raw = rng.integers(0, 65536, size=(96, 128), dtype=np.uint16)
    for out_size in ((64, 48), (50, 31), (200, 150)):
        d, c = _run(raw, col, 5000.0, 0, out_size)
        de, ce = _expected(raw, col, 5000.0, 0, out_size)
        assert torch.equal(d, de) and torch.equal(c, ce), out_size


@pytest.mark.parametrize("in_size, out_size", [((96, 1024), (48, 32)), ((1024, 96), (32, 48)), ((70, 1000), (70, 10))])
def test_large_reduction_shrinks_the_tile(in_size, out_size):
    """Reduction factors of 32 and 100: a 16-row tile's source rows no longer fit the LDS, the tile height drops (to 4, and
    to 1 for 100: y_ksize 201, 202 staged rows of 256 B), the windows stay whole."""
    rng = np.random.default_rng(in_size[0])
    raw, col = _frame(rng, in_size[0], in_size[1], 3, 0)
    d, c = _run(raw, col, 1000.0, 0, out_size)
    de, ce = _expected(raw, col, 1000.0, 0, out_size)
    assert torch.equal(d, de) and torch.equal(c, ce)


def test_same_size_takes_the_plain_path():
    rng = np.random.default_rng(2)
    raw, col = _frame(rng, 120, 68, 3, 8)
    d0, c0 = ds.ingest(torch.from_numpy(raw.view(np.int16)).to(DEV), torch.from_numpy(col).to(DEV), 6553.5, 8)
    d1, c1 = _run(raw, col, 6553.5, 8, (120, 68))
    assert torch.equal(d0, d1) and torch.equal(c0, c1)


def test_bad_arguments_are_rejected():
    raw = torch.zeros(16, 16, dtype=torch.int16, device=DEV)
    col = torch.zeros(16, 16, 3, dtype=torch.uint8, device=DEV)
    for bad in ((0, 8), (8, 0), (-4, 8)):
        with pytest.raises(ValueError, match="out_size"):
            ds.ingest(raw, col, 1000.0, 0, out_size=bad)
    good = ds.resize_tables((16, 16), (8, 8)).to(DEV)
    with pytest.raises(ValueError, match="tables"):                            # tables of another size pair
        ds.ingest(raw, col, 1000.0, 0, out_size=(8, 8), tables=ds.resize_tables((16, 16), (4, 4)).to(DEV))
    import dataclasses
    short = dataclasses.replace(good, device_buf=good.device_buf[:-1].contiguous())
    with pytest.raises(ValueError, match="resize tables"):                     # tables of the wrong length
        ds.ingest(raw, col, 1000.0, 0, out_size=(8, 8), tables=short)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ds.ingest(raw, col, 0.0, 0, out_size=(8, 8), tables=good)
    # the entry point itself: a wrong tables_len, a zero output side and a null table pointer return -1 before any launch
    from rtg_slam_amd import _lib
    lib = _lib.load()
    d = torch.full((8, 8), 7.0, device=DEV)
    c = torch.full((3, 8, 8), 7.0, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())
    buf, n = good.device_buf, int(good.device_buf.numel())
    call = lambda Ho, Wo, tab, length: lib.rtgs_ingest_rgbd_resized(P(raw), P(col), 16, 16, 3, 0, 1000.0, Ho, Wo, tab, length,
                                                                      good.x_ksize, good.y_ksize, P(d), P(c), None)
    assert call(8, 8, P(buf), n - 1) == -1 and call(0, 8, P(buf), n) == -1 and call(8, 8, None, n) == -1
    # a window that does not fit the LDS: 8192 rows to 8 (y_ksize 2049)
    tall_raw = torch.zeros(8192, 8, dtype=torch.int16, device=DEV)
    tall_col = torch.zeros(8192, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ds.ingest(tall_raw, tall_col, 1000.0, 0, out_size=(8, 8))
    torch.cuda.synchronize()
    assert float(d.min()) == float(d.max()) == 7.0 and float(c.min()) == float(c.max()) == 7.0      # nothing was launched
    assert call(8, 8, P(buf), n) == 0                                          # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert float(c.max()) == 0.0


def _replica_dataset(root, n=10, H=68, W=120):
    rng = np.random.default_rng(5)
    scene = os.path.join(root, "Replica", "room")
    os.makedirs(os.path.join(scene, "results"))
    lines = []
    for i in range(n):
        raw = rng.integers(0, 65536, size=(H, W), dtype=np.uint16)
        Image.fromarray(raw).save(os.path.join(scene, "results", f"depth{i:06d}.png"))
        Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(
            os.path.join(scene, "results", f"frame{i:06d}.jpg"), quality=90)
        P = np.eye(4)
        P[:3, 3] = rng.normal(size=3)
        lines.append(" ".join(repr(float(v)) for v in P.reshape(-1)))
    open(os.path.join(scene, "traj.txt"), "w").write("\n".join(lines) + "\n")
    json.dump({"camera": {"w": W, "h": H, "fx": 60.0, "fy": 60.0, "cx": 59.5, "cy": 33.5, "scale": 6553.5}},
              open(os.path.join(root, "Replica", "cam_params.json"), "w"))
    return scene


@pytest.mark.parametrize("workers, prefetch", [(1, 1), (None, None)])
def test_frame_source_resized_in_order_and_equal(tmp_path, workers, prefetch):
    info = ds.resize_info(ds.read_replica(_replica_dataset(str(tmp_path))), 2.0)
    assert (info.width, info.height, info.raw_width, info.raw_height) == (60, 34, 120, 68)
    src = ds.FrameSource(info, DEV, io_workers=workers, prefetch=prefetch)
    got = 0
    for _ in range(2):                                               # a source can be iterated again
        for i, (d, c, c2w) in enumerate(src):
            rec = info.frames[i]
            raw = ds.decode_depth(rec.depth_path)
            col = ds.decode_color(rec.color_path, info.raw_width, info.raw_height)
            de, ce = _expected(raw, col, info.depth_scale, 0, (60, 34))
            assert d.device == c.device == DEV and d.shape == (34, 60, 1) and c.shape == (3, 34, 60)
            assert torch.equal(d, de) and torch.equal(c, ce), i
            assert np.array_equal(c2w, rec.c2w)
            got += 1
        st = src.stats()
        assert st["frames"] == 10 and st["h2d_bytes_per_frame"] == 68 * 120 * 5        # the raw frame travels
        assert (st["width"], st["height"], st["resolution_scale"]) == (60, 34, 2.0)
    assert got == 20


def test_frame_source_default_settings_unchanged(tmp_path):
    from types import SimpleNamespace
    scene = _replica_dataset(str(tmp_path), n=4)
    info = ds.load_dataset(SimpleNamespace(type="Replica", source_path=scene, resolution=1, resolution_scales=[1.0]))
    assert not info.resized
    src = ds.FrameSource(info, DEV, io_workers=2)
    for i, (d, c, _) in enumerate(src):
        rec = info.frames[i]
        raw = torch.from_numpy(ds.decode_depth(rec.depth_path).copy().view(np.int16)).to(DEV)
        col = torch.from_numpy(ds.decode_color(rec.color_path, 120, 68).copy()).to(DEV)
        d0, c0 = ds.ingest(raw, col, info.depth_scale, 0)            # rtgs_ingest_rgbd
        assert torch.equal(d, d0) and torch.equal(c, c0)
    assert src._tables is None and (src.stats()["width"], src.stats()["height"]) == (120, 68)


# ------------------------------------------------------------------------------------------------------------ end to end
N = 20
ATE_MEASURED_CM = 0.0141      # the final ATE of this run measured on the MI355X, see the test's docstring


def _write_full_dataset(root):
    cam = synth.REPLICA
    scene = os.path.join(root, "Replica", "room0")
    os.makedirs(os.path.join(scene, "results"))
    lines = []
    for i, p in enumerate(synth.trajectory(N, seed=21)):
        d = synth.box_room_depth(cam, p, device=DEV)
        col = synth.box_room_color(cam, p, d)
        raw = torch.clamp(torch.round(d[..., 0].double() * 6553.5), 0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)
        rgb = torch.clamp(torch.round(col.permute(1, 2, 0).double() * 255), 0, 255).to(torch.uint8).cpu().numpy()
        Image.fromarray(raw).save(os.path.join(scene, "results", f"depth{i:06d}.png"))
        Image.fromarray(rgb).save(os.path.join(scene, "results", f"frame{i:06d}.jpg"), quality=95)
        lines.append(" ".join(repr(float(v)) for v in p.numpy().reshape(-1)))
    open(os.path.join(scene, "traj.txt"), "w").write("\n".join(lines) + "\n")
    json.dump({"camera": {"w": cam.W, "h": cam.H, "fx": cam.fx, "fy": cam.fy, "cx": cam.cx, "cy": cam.cy, "scale": 6553.5}},
              open(os.path.join(root, "Replica", "cam_params.json"), "w"))
    return scene


def _config(root, scene, save):
    base = os.path.join(ROOT, "tests", "golden", "configs", "replica_base.yaml")
    path = os.path.join(root, "run.yaml")
    # the overrides tests/test_run_config_gpu.py uses for its half-size frames
    open(path, "w").write(f"""parent: "{base}"
source_path: "{scene}"
save_path: "{save}"
save_step: 10
frame_start: 0
frame_step: 0
frame_num: -1
uniform_sample_num: 10200
gaussian_update_iter: 30
stable_confidence_thres: 40.0
unstable_time_window: 24
max_depth: 8.0
keyframe_trans_thes: 0.25
seed: 1
""")
    return path


def _cli(argv, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "rtg_slam_amd"] + argv, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_slam_then_metric_at_half_size(tmp_path):
    """`slam --resolution-scale 2` and `metric --resolution-scale 2` on the box room written at the full 1200 x 680: the run
    sees 600 x 340 frames (antialiased colour, nearest-picked depth) and the reference's resized camera.

    ATE bound: twice the final ATE measured for this very run on the MI355X: 0.0141 cm (six runs: 0.01409 - 0.01429 cm,
    profiles/r10_resize_e2e_ate.json), so ate[-1] < 0.0282 cm.  The measured value itself must stay far below the config's
    25 cm keyframe translation threshold for "tracking held" to mean anything; the test asserts that as < 2.5 cm.  (The
    half-size dataset of tests/test_run_config_gpu.py, rendered directly at 600 x 340, is accepted there below 1 cm.)"""
    scene = _write_full_dataset(str(tmp_path))
    save = os.path.join(str(tmp_path), "out")
    cfg = _config(str(tmp_path), scene, save)
    out = _cli(["slam", "--config", cfg, "--io-workers", "4", "--resolution-scale", "2"], 900)
    assert "600x340" in out and "1200x680" in out
    import yaml
    merged = yaml.safe_load(open(os.path.join(save, "config.yaml")))
    assert merged["resolution_scales"] == [2.0] and merged["resolution"] == 1
    rep = json.load(open(os.path.join(save, "run_report.json")))
    assert (rep["width"], rep["height"], rep["resolution_scale"]) == (600, 340, 2.0) and rep["frames"] == N
    assert rep["h2d_bytes_per_frame"] == 1200 * 680 * 5
    es = np.load(os.path.join(save, "save_traj", "pose_es.npy"))
    gt = np.load(os.path.join(save, "save_traj", "pose_gt.npy"))
    assert es.shape == gt.shape == (N, 4, 4)
    ate = [float(x) for x in open(os.path.join(save, "save_traj", "ate.txt")).read().split()]
    print(f"final ATE at half size: {ate[-1]!r} cm")
    assert len(ate) == N

    _cli(["metric", "--config", cfg, "--resolution-scale", "2"], 600)
    final = os.path.join(save, "save_model", f"frame_{N:04d}")
    csvs = [n for n in os.listdir(save) if n.startswith(f"statis_frame_{N}_iter_")]
    assert len(csvs) == 1, csvs
    with open(os.path.join(save, csvs[0])) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == N + 1 and rows[-1]["frame"] == "mean"

    # the same evaluation in process at 600 x 340, on the same model file
    from rtg_slam_amd import __main__ as cli, config, evaluation
    args = config.load_config(os.path.join(save, "config.yaml"))         # carries resolution_scales: [2.0]
    model = cli.filter_models(final, False, [])[0]
    mapper = cli.load_map(args, DEV, os.path.join(final, model))
    args.frame_num = N
    info = ds.load_dataset(args)
    assert (info.width, info.height) == (600, 340)
    res = evaluation.evaluate_sequence(mapper, info.camera(), ds.FrameSource(info, DEV), poses=es, args=args)
    assert len(res["rows"]) == N
    for row, want in zip(rows[:N], res["rows"]):
        assert int(row["frame"]) == want["frame"]
        for k in ("psnr", "ssim", "depth_loss", "valid_pixel_ratio", "color_l1"):
            a, b = float(row[k]), float(want[k])
            assert abs(a - b) <= 1e-5 * max(abs(b), 1e-12), (k, row["frame"], a, b)
    assert ATE_MEASURED_CM is not None and ATE_MEASURED_CM < 2.5
    assert ate[-1] < 2 * ATE_MEASURED_CM, ate[-1]
