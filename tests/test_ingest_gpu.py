"""The frame ingest kernel (rtgs_ingest_rgbd) and the streaming frame source against the reference's float chain on the CPU
(numpy float32 depth scaling, PILtoTorch's / 255 in torch, map_preprocess's * 255 on the device): torch.equal everywhere."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from rtg_slam_amd import datasets as ds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _expected(raw, col, scale, crop):
    d, c = ds.reference_chain(raw, col, scale, crop)
    return (d.to(DEV) * 255).unsqueeze(-1), c.contiguous().to(DEV)      # tracker.py:97-101: * 255 on the GPU, [H,W,1]


def _run(raw, col, scale, crop):
    return ds.ingest(torch.from_numpy(raw.view(np.int16)).to(DEV), torch.from_numpy(col).to(DEV), scale, crop)


@pytest.mark.parametrize("crop", [0, 8])
@pytest.mark.parametrize("scale", [6553.5, 5000.0, 1000.0])
def test_every_depth_value_and_scale(scale, crop):
    n = 256 + 2 * crop
    rng = np.random.default_rng(crop)
    raw = rng.integers(0, 65536, size=(n, n), dtype=np.uint16)
    raw[crop:crop + 256, crop:crop + 256] = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    col = rng.integers(0, 256, size=(n, n, 3), dtype=np.uint8)
    d, c = _run(raw, col, scale, crop)
    torch.cuda.synchronize()
    de, ce = _expected(raw, col, scale, crop)
    assert d.shape == (256, 256, 1) and c.shape == (3, 256, 256) and d.dtype == c.dtype == torch.float32
    assert torch.equal(d, de) and torch.equal(c, ce)


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("crop", [0, 8])
def test_every_colour_value(channels, crop):
    n = 64 + 2 * crop
    rng = np.random.default_rng(channels)
    col = rng.integers(0, 256, size=(n, n, channels), dtype=np.uint8)
    inner = np.arange(64 * 64 * channels) % 256
    col[crop:crop + 64, crop:crop + 64] = rng.permutation(inner).astype(np.uint8).reshape(64, 64, channels)
    raw = rng.integers(0, 65536, size=(n, n), dtype=np.uint16)
    d, c = _run(raw, col, 6553.5, crop)
    de, ce = _expected(raw, col, 6553.5, crop)
    assert torch.equal(d, de) and torch.equal(c, ce)
    assert set(np.unique(col[crop:crop + 64, crop:crop + 64, :3]).tolist()) == set(range(256))


@pytest.mark.parametrize("shape, crop, channels", [((7, 13), 0, 3), ((7, 13), 1, 4), ((23, 21), 8, 3),
                                                   ((680, 1200), 0, 3), ((680, 1200), 8, 4), ((680, 1202), 0, 3)])
def test_odd_and_full_sizes(shape, crop, channels):
    rng = np.random.default_rng(shape[0] * 7 + crop)
    raw = rng.integers(0, 65536, size=shape, dtype=np.uint16)
    col = rng.integers(0, 256, size=shape + (channels,), dtype=np.uint8)
    for scale in (6553.5, 5000.0):
        d, c = _run(raw, col, scale, crop)
        de, ce = _expected(raw, col, scale, crop)
        assert torch.equal(d, de) and torch.equal(c, ce)


def test_bad_arguments_are_rejected():
    raw = torch.zeros(8, 8, dtype=torch.int16, device=DEV)
    col = torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ds.ingest(raw, col, 1000.0, 4)                               # nothing left after the crop
    with pytest.raises(ValueError):
        ds.ingest(raw, torch.zeros(8, 8, 2, dtype=torch.uint8, device=DEV), 1000.0, 0)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ds.ingest(raw, col, 0.0, 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ds.ingest(raw.cpu(), col.cpu(), 1000.0, 0)


def _replica_dataset(root, n=10, H=68, W=120):
    rng = np.random.default_rng(5)
    scene = os.path.join(root, "Replica", "room")
    os.makedirs(os.path.join(scene, "results"))
    raws, lines = [], []
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


@pytest.mark.parametrize("workers, prefetch", [(1, 1), (None, None), (3, 2)])
def test_frame_source_in_order_and_equal(tmp_path, workers, prefetch):
    info = ds.read_replica(_replica_dataset(str(tmp_path)))
    src = ds.FrameSource(info, DEV, io_workers=workers, prefetch=prefetch)
    got = 0
    for _ in range(2):                                               # a source can be iterated again
        for i, (d, c, c2w) in enumerate(src):
            rec = info.frames[i]
            raw = ds.decode_depth(rec.depth_path)
            col = ds.decode_color(rec.color_path, info.raw_width, info.raw_height)
            de, ce = _expected(raw, col, info.depth_scale, 0)
            assert d.device == c.device == DEV and d.shape == (info.height, info.width, 1) and c.shape == (3, info.height, info.width)
            assert torch.equal(d, de) and torch.equal(c, ce), i
            assert isinstance(c2w, np.ndarray) and c2w.dtype == np.float64 and np.array_equal(c2w, rec.c2w)
            got += 1
        st = src.stats()
        assert st["frames"] == len(info) == 10 and st["h2d_bytes_per_frame"] == info.raw_height * info.raw_width * 5
        assert st["io_wait_s"] >= 0 and st["decode_ms_per_frame"] > 0
    assert got == 20


def test_frame_source_stops_early_and_is_consumed_on_another_stream(tmp_path):
    info = ds.read_replica(_replica_dataset(str(tmp_path), n=6))
    src = ds.FrameSource(info, DEV, io_workers=2, prefetch=3)
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        it = iter(src)
        d, c, _ = next(it)
        total = (d.sum() + c.sum())                                  # ordered after the ingest by the event wait
        it.close()                                                   # pending decodes are cancelled / drained
    torch.cuda.synchronize()
    raw = ds.decode_depth(info.frames[0].depth_path)
    col = ds.decode_color(info.frames[0].color_path, info.raw_width, info.raw_height)
    de, ce = _expected(raw, col, info.depth_scale, 0)
    assert torch.equal(total, de.sum() + ce.sum())
