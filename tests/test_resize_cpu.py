"""The host side of the resized ingest: resample_tables / nearest_indices / reference_resize against the installed Pillow
(bit for bit: np.array_equal, no pixel left out), loadCam's output size and the resized intrinsics against values worked out
by hand from utils/camera_utils.py:22-74 and scene/cameras.py, and load_dataset's handling of resolution / resolution_scales."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from rtg_slam_amd import datasets as ds

# (W, H) -> (Wo, Ho)
SIZE_PAIRS = [((1200, 680), (600, 340)), ((1200, 680), (300, 170)), ((640, 480), (320, 240)), ((601, 337), (400, 225)),
              ((320, 200), (320, 100)), ((320, 200), (160, 200)), ((100, 60), (250, 171)), ((1184, 664), (592, 332)),
              ((37, 23), (5, 3)), ((64, 48), (7, 48))]


def _pil_color(a, size):
    return np.array(Image.fromarray(a).resize(size, Image.BILINEAR))


def _pil_depth(d, size):
    return np.array(Image.fromarray(d).resize(size, Image.NEAREST))


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("in_size, out_size", SIZE_PAIRS)
def test_reference_resize_equals_pillow(in_size, out_size, channels):
    (W, H), (Wo, Ho) = in_size, out_size
    rng = np.random.default_rng(W * 31 + Ho + channels)
    a = rng.integers(0, 256, size=(H, W, channels), dtype=np.uint8)
    d = (rng.integers(0, 65536, size=(H, W)).astype(np.float32) / np.float32(6553.5))
    assert Image.fromarray(a).mode == ("RGB" if channels == 3 else "RGBA") and Image.fromarray(d).mode == "F"
    c, dd = ds.reference_resize(a, d, Wo, Ho)
    assert c.dtype == np.uint8 and c.shape == (Ho, Wo, channels) and dd.dtype == np.float32 and dd.shape == (Ho, Wo)
    assert np.array_equal(c, _pil_color(a, (Wo, Ho)))
    assert np.array_equal(dd, _pil_depth(d, (Wo, Ho)))


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("value", [0, 255])
@pytest.mark.parametrize("in_size, out_size", [((1200, 680), (600, 340)), ((601, 337), (400, 225)), ((100, 60), (250, 171))])
def test_constant_images(in_size, out_size, value, channels):
    (W, H), (Wo, Ho) = in_size, out_size
    a = np.full((H, W, channels), value, dtype=np.uint8)
    c, _ = ds.reference_resize(a, None, Wo, Ho)
    assert np.array_equal(c, _pil_color(a, (Wo, Ho)))
    assert (c == value).all()                                       # the fixed-point weights lose nothing at either end


def test_rgba_with_structured_alpha():
    """Alpha 0, 255 and everything between, next to each other: the premultiply / divide round trip of Image.resize."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(96, 128, 4), dtype=np.uint8)
    a[:32, :, 3] = 0
    a[32:64, :, 3] = 255
    a[64:, :, 3] = np.arange(128, dtype=np.uint8)[None, :] * 2
    for size in ((64, 48), (50, 31), (200, 150)):
        c, _ = ds.reference_resize(a, None, *size)
        assert np.array_equal(c, _pil_color(a, size)), size


def test_tables_shape_and_windows():
    for n_in, n_out in ((1200, 600), (680, 170), (337, 225), (60, 171), (200, 200)):
        start, length, coeff = ds.resample_tables(n_in, n_out)
        near = ds.nearest_indices(n_in, n_out)
        ksize = int(np.ceil(max(n_in / n_out, 1.0))) * 2 + 1
        assert start.dtype == length.dtype == coeff.dtype == near.dtype == np.int32
        assert start.shape == length.shape == near.shape == (n_out,) and coeff.shape == (n_out, ksize)
        assert (start >= 0).all() and (length >= 1).all() and (start + length <= n_in).all() and length.max() <= ksize
        assert (np.diff(start) >= 0).all() and (np.diff(start + length) >= 0).all()       # what the kernel's tiling relies on
        assert (coeff >= 0).all() and (coeff[np.arange(ksize)[None, :] >= length[:, None]] == 0).all()
        assert np.abs(coeff.sum(1) - (1 << ds.RESAMPLE_BITS)).max() <= ksize             # weights sum to 1 up to rounding
        assert (near >= 0).all() and (near < n_in).all() and (np.diff(near) >= 0).all()
    t = ds.resize_tables((1200, 680), (600, 340))
    assert (t.x_ksize, t.y_ksize) == (5, 5) and t.packed.dtype == np.int32 and t.packed.shape == (t.expected_len(),)
    assert t.expected_len() == 3 * 600 + 3 * 340 + 600 * 5 + 340 * 5
    with pytest.raises(ValueError):
        ds.resample_tables(0, 4)
    with pytest.raises(ValueError):
        ds.nearest_indices(4, 0)


# loadCam: resolution in [1, 2, 4, 8] -> round(orig / (resolution_scale * resolution)) per axis (Python's round: ties to even);
# otherwise int(orig / (global_down * resolution_scale)).
@pytest.mark.parametrize("size, scale, want", [
    ((1200, 680), 1.0, (1200, 680)), ((1200, 680), 2.0, (600, 340)), ((1200, 680), 4.0, (300, 170)), ((1200, 680), 1.5, (800, 453)),
    ((1184, 664), 2.0, (592, 332)), ((1184, 664), 4.0, (296, 166)), ((1184, 664), 1.5, (789, 443)),
    ((601, 337), 2.0, (300, 168)),            # 300.5 and 168.5: round goes to the even neighbour
    ((603, 339), 2.0, (302, 170)),            # 301.5 -> 302, 169.5 -> 170: int() would give 301, 169
    ((601, 337), 1.5, (401, 225)),            # 400.67 and 224.67: int() would give 400, 224
    ((624, 464), 4.0, (156, 116)),
])
def test_loadcam_size_by_hand(size, scale, want):
    assert ds.loadcam_size(size[0], size[1], 1, scale) == want
    assert all(isinstance(v, int) for v in ds.loadcam_size(size[0], size[1], 1, scale))


def test_loadcam_size_int_branch():
    assert ds.loadcam_size(601, 337, -1, 1.5) == (400, 224)           # resolution -1 on a narrow frame: global_down 1, int()
    assert ds.loadcam_size(603, 339, 603, 2.0) == (301, 169)          # resolution == width: global_down 1, int()


def _info(W, H, crop, fx, fy, cx, cy):
    fr = ds.FrameRecord("c.jpg", "d.png", np.eye(4), 0.0, "c")
    return ds.DatasetInfo("TUM", "/nowhere", [fr], fx, fy, cx - crop, cy - crop, 5000.0, crop, H, W)


# Camera(FoVx = focal2fov(fx, W)) keeps the field of view, and the loop reads fx back as fov2focal(FoVx, Wo): since
# tan(atan(t)) = t, fx' = Wo / (2 * W / (2 fx)) = fx Wo / W exactly in real numbers (the same for fy with H, Ho); the float64
# atan / tan round trip is good to a few ulp, hence rel 1e-12.  cx' = cx / resolution_scale, cy' = cy / resolution_scale.
@pytest.mark.parametrize("crop", [0, 8])
@pytest.mark.parametrize("scale", [1.0, 2.0, 4.0, 1.5])
@pytest.mark.parametrize("raw, K", [((640, 480), (517.3, 516.5, 318.6, 255.3)), ((1200, 680), (600.0, 600.0, 599.5, 339.5)),
                                    ((603, 339), (410.0, 395.5, 300.25, 170.75))])
def test_resized_intrinsics_by_hand(raw, K, scale, crop):
    Wd, Hd = raw
    fx, fy, cx, cy = K
    info = _info(Wd, Hd, crop, fx, fy, cx, cy)
    W, H = Wd - 2 * crop, Hd - 2 * crop
    assert (info.width, info.height, info.crop_width, info.crop_height) == (W, H, W, H) and not info.resized
    out = ds.resize_info(info, scale)
    Wo, Ho = round(W / scale), round(H / scale)
    assert (out.width, out.height) == (Wo, Ho) and (out.crop_width, out.crop_height) == (W, H)
    assert (out.raw_width, out.raw_height, out.crop_edge) == (Wd, Hd, crop) and out.resolution_scale == scale
    if scale == 1.0:
        assert out is info
        return
    assert out.resized and info.out_width is None                     # the input is not modified
    assert out.fx == pytest.approx(fx * Wo / W, rel=1e-12) and out.fy == pytest.approx(fy * Ho / H, rel=1e-12)
    assert out.cx == (cx - crop) / scale and out.cy == (cy - crop) / scale
    cam = out.camera()
    assert (cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy) == (Ho, Wo, out.fx, out.fy, out.cx, out.cy)


def test_resized_intrinsics_literal():
    """One case in plain numbers: a 1200 x 680 Replica camera at scale 2."""
    fx, fy, cx, cy = ds.resized_intrinsics(600.0, 600.0, 599.5, 339.5, 1200, 680, 600, 340, 2.0)
    assert fx == pytest.approx(300.0, rel=1e-12) and fy == pytest.approx(300.0, rel=1e-12) and (cx, cy) == (299.75, 169.75)
    with pytest.raises(ValueError):
        ds.resize_info(_info(64, 48, 0, 50.0, 50.0, 31.5, 23.5), 0.0)
    with pytest.raises(ValueError):
        ds.resize_info(_info(64, 48, 0, 50.0, 50.0, 31.5, 23.5), 1000.0)       # nothing left


def _replica(root, n=4, W=24, H=16):
    rng = np.random.default_rng(1)
    scene = os.path.join(root, "Replica", "office0")
    os.makedirs(os.path.join(scene, "results"))
    lines = []
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(f"{scene}/results/frame{i:06d}.jpg")
        Image.fromarray(rng.integers(0, 65536, size=(H, W), dtype=np.uint16)).save(f"{scene}/results/depth{i:06d}.png")
        P = np.eye(4)
        P[:3, 3] = rng.normal(size=3)
        lines.append(" ".join(repr(float(v)) for v in P.reshape(-1)))
    open(f"{scene}/traj.txt", "w").write("\n".join(lines) + "\n")
    json.dump({"camera": {"w": W, "h": H, "fx": 20.5, "fy": 21.75, "cx": 11.5, "cy": 7.25, "scale": 6553.5}},
              open(os.path.join(root, "Replica", "cam_params.json"), "w"))
    return scene


def test_load_dataset_resolution_scales(tmp_path):
    scene = _replica(str(tmp_path))
    base = dict(type="Replica", source_path=scene, frame_start=0, frame_num=-1, frame_step=0, eval=False, resolution=1,
                resolution_scales=[1.0])
    plain = ds.read_replica(scene)
    info = ds.load_dataset(SimpleNamespace(**base))                    # the defaults: exactly what the reader returns
    assert (info.width, info.height, info.raw_width, info.raw_height) == (24, 16, 24, 16) and not info.resized
    assert (info.fx, info.fy, info.cx, info.cy) == (plain.fx, plain.fy, plain.cx, plain.cy) == (20.5, 20.5, 11.5, 7.25)
    assert info.resolution_scale == 1.0 and info.out_width is None and info.out_height is None and len(info) == 4
    assert [f.depth_path for f in info.frames] == [f.depth_path for f in plain.frames]
    assert all(np.array_equal(a.c2w, b.c2w) for a, b in zip(info.frames, plain.frames))

    half = ds.load_dataset(SimpleNamespace(**{**base, "resolution_scales": [2.0]}))
    assert (half.width, half.height) == (12, 8) and (half.raw_width, half.raw_height) == (24, 16) and half.resized
    assert half.fx == pytest.approx(10.25, rel=1e-12) and half.fy == pytest.approx(10.25, rel=1e-12)
    assert (half.cx, half.cy) == (5.75, 3.625) and half.resolution_scale == 2.0
    assert [f.color_path for f in half.frames] == [f.color_path for f in info.frames]
    cam = half.camera()
    assert (cam.H, cam.W, cam.cx, cam.cy) == (8, 12, 5.75, 3.625)
    third = ds.load_dataset(SimpleNamespace(**{**base, "resolution_scales": [1.5, 3.0]}))    # only the first entry counts
    assert (third.width, third.height) == (16, 11)                    # round(10.67) = 11
    up = ds.load_dataset(SimpleNamespace(**{**base, "resolution_scales": [0.5]}))
    assert (up.width, up.height) == (48, 32) and (up.cx, up.cy) == (23.0, 14.5)
    # a resolution that by itself keeps the size is accepted, and selects loadCam's int() branch
    same = ds.load_dataset(SimpleNamespace(**{**base, "resolution": -1, "resolution_scales": [1.5]}))
    assert (same.width, same.height) == (16, 10)                      # int(10.67) = 10

    for scales in ([1.0], [2.0], [0.5]):                              # `resolution` alone must not resize: cx, cy would be wrong
        with pytest.raises(ValueError, match="would resize") as e:
            ds.load_dataset(SimpleNamespace(**{**base, "resolution": 2, "resolution_scales": scales}))
        assert "resolution_scales" in str(e.value)
    with pytest.raises(ValueError, match="would resize"):
        ds.load_dataset(SimpleNamespace(**{**base, "resolution": 12}))
    with pytest.raises(ValueError):
        ds.load_dataset(SimpleNamespace(**{**base, "resolution_scales": [0.0]}))
    with pytest.raises(ValueError, match="eval"):
        ds.load_dataset(SimpleNamespace(**{**base, "eval": True, "resolution_scales": [2.0]}))


def test_cli_resolution_scale_option():
    from rtg_slam_amd import __main__ as cli
    p = cli.build_parser()
    for cmd in ("slam", "metric"):
        assert p.parse_args([cmd, "--config", "x.yaml"]).resolution_scale is None
        o = p.parse_args([cmd, "--config", "x.yaml", "--resolution-scale", "2"])
        assert o.resolution_scale == 2.0
        args = SimpleNamespace(resolution_scales=[1.0, 4.0])
        cli._apply_resolution_scale(args, o)
        assert args.resolution_scales == [2.0, 4.0]
    args = SimpleNamespace()
    cli._apply_resolution_scale(args, p.parse_args(["slam", "--config", "x.yaml", "--resolution-scale", "1.5"]))
    assert args.resolution_scales == [1.5]
