"""Recorded RGB-D datasets in the reference's layouts, and the streaming frame source that feeds `slam.run_sequence` from them.

Readers (the live paths of scene/dataset_readers.py: sceneLoadTypeCallbacks :1076-1083, every one ending in readCameras
:848-932; readReplicaCameras / readTumCameras are never called and are not restated):

    read_replica    readReplicaSceneInfo :774-846   results/frame*.jpg, results/depth*.png, traj.txt, ../cam_params.json
    read_tum        readTumSceneInfo     :545-690   rgb.txt, depth.txt, groundtruth.txt | pose.txt, config.yaml
    read_ours       readOursSceneInfo    :968-1074  color/*.jpg, depth/*.png, pose/*.txt, intrinsic/intrinsic_depth.txt
                                                    (type "Ours" and "Scannetpp")

Each returns a `DatasetInfo`: the selected frames in the order the reference's loop sees them (file paths, camera-to-world
pose relative to the first selected frame, timestamp), the intrinsics after the crop, the depth scale and the frame size.
No image is decoded there except the first depth's header (the frame size).

`FrameSource` iterates the frames as (depth [H,W,1] metres, colour [3,H,W] in 0..1, ground-truth c2w float64 4x4), the
tensors on the device, as run_sequence consumes them.  Decoding (PIL + numpy) runs on a pool of worker threads; each
decoded frame's raw bytes (u16 depth, u8 colour: 6 B per pixel for RGB) go through a ring of pinned host buffers to the
device on a dedicated stream, where one `rtgs_ingest_rgbd` launch turns them into the float maps, bit-identical to the
reference's chain (include/rtgs_slam.h, "frame ingest").  Frames come out in dataset order.

With `resolution_scales: [S]`, S != 1, the frames are resized after the crop as utils/camera_utils.py:22-74 (loadCam) resizes
them: the raw frame still travels to the device, where one `rtgs_ingest_rgbd_resized` launch reproduces PIL's BILINEAR
(colour) and NEAREST (depth) resize bit for bit from tables computed here in float64 (resample_tables, nearest_indices);
`DatasetInfo.width / height / camera()` then describe the resized frames (resize_info)."""
from __future__ import annotations

import ctypes as C
import dataclasses
import glob
import json
import math
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

MAX_IO_WORKERS = 16                       # a command on the GPU hosts gets 16 CPUs


@dataclass
class FrameRecord:
    color_path: str
    depth_path: str
    c2w: np.ndarray                       # float64 [4,4], relative to the first selected frame (readCameras' pose_w_t0)
    timestamp: float
    image_name: str


@dataclass
class DatasetInfo:
    type: str
    source_path: str
    frames: List[FrameRecord]
    fx: float
    fy: float
    cx: float                             # after the crop: cx - crop_edge (and after the resize, when there is one)
    cy: float
    depth_scale: float
    crop_edge: int
    raw_height: int                       # the depth image's size (colour is resized to it)
    raw_width: int
    mesh_path: Optional[str] = None
    extra: dict = field(default_factory=dict)
    resolution_scale: float = 1.0         # loadCam's resolution_scale; fx, fy, cx, cy describe the frames AFTER the resize
    out_width: Optional[int] = None       # the size loadCam resizes the cropped frames to; None: the cropped size
    out_height: Optional[int] = None

    @property
    def crop_height(self) -> int:
        return self.raw_height - 2 * self.crop_edge

    @property
    def crop_width(self) -> int:
        return self.raw_width - 2 * self.crop_edge

    @property
    def height(self) -> int:
        return self.crop_height if self.out_height is None else int(self.out_height)

    @property
    def width(self) -> int:
        return self.crop_width if self.out_width is None else int(self.out_width)

    @property
    def resized(self) -> bool:
        return (self.width, self.height) != (self.crop_width, self.crop_height)

    def camera(self):
        from .synth import CameraSpec
        return CameraSpec(self.height, self.width, self.fx, self.fy, self.cx, self.cy)

    def __len__(self) -> int:
        return len(self.frames)


# --------------------------------------------------------------------------------------------------------------- readers
def _select(n_img: int, frame_start: int, frame_num: int, frame_step: int) -> List[int]:
    """frame_start + i * (frame_step + 1) for i < frame_num (all n_img when frame_num == -1), bounded by n_img."""
    count = n_img if frame_num == -1 else int(frame_num)
    idx = [int(frame_start) + i * (int(frame_step) + 1) for i in range(count)]
    return [i for i in idx if i < n_img]


def _image_size(path: str):
    from PIL import Image
    with Image.open(path) as im:
        return im.size                                            # (w, h)


def read_cameras(type_: str, source_path: str, color_paths, depth_paths, poses, intrinsic, indices, depth_scale, timestamps,
                 crop_edge: int = 0, mesh_path=None) -> DatasetInfo:
    """readCameras (:848-932) without decoding: pose_w_t0 = inverse of the FIRST selected pose (taken before the inf test);
    a pose with inf in it is skipped; every kept pose becomes pose_w_t0 @ c2w; cx, cy shift by crop_edge."""
    frames: List[FrameRecord] = []
    pose_w_t0 = np.eye(4)
    for k, idx in enumerate(indices):
        c2w = np.asarray(poses[idx], dtype=np.float64)
        if k == 0:
            pose_w_t0 = np.linalg.inv(c2w)
        if np.isinf(c2w).any():
            continue
        c2w = pose_w_t0 @ c2w
        frames.append(FrameRecord(color_paths[idx], depth_paths[idx], c2w, float(timestamps[idx]),
                                  os.path.basename(color_paths[idx]).split(".")[0]))
    if not frames:
        raise ValueError(f"rtg_slam_amd.datasets: no frame selected from {source_path}")
    w, h = _image_size(frames[0].depth_path)
    c = int(crop_edge)
    if c < 0 or h - 2 * c <= 0 or w - 2 * c <= 0:
        raise ValueError(f"rtg_slam_amd.datasets: crop_edge {c} does not fit a {w}x{h} frame")
    K = np.asarray(intrinsic, dtype=np.float64)
    return DatasetInfo(type_, source_path, frames, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]) - c, float(K[1, 2]) - c,
                       float(depth_scale), c, int(h), int(w), mesh_path)


def read_replica(datapath: str, frame_start: int = 0, frame_num: int = -1, frame_step: int = 0) -> DatasetInfo:
    """readReplicaSceneInfo (:774-846): poses from traj.txt (one row-major 4x4 per line) relative to its first line;
    intrinsics from ../cam_params.json["camera"] with fy := fx (:805-808), depth scale "scale".  Unlike the reference, the
    selected indices are bounded by the number of frames (as the TUM and Ours readers do): frame_start / frame_step running
    past the end select fewer frames instead of raising IndexError."""
    color_paths = sorted(glob.glob(f"{datapath}/results/frame*.jpg"))
    depth_paths = sorted(glob.glob(f"{datapath}/results/depth*.png"))
    n_img = len(color_paths)
    if n_img == 0 or len(depth_paths) < n_img:
        raise FileNotFoundError(f"rtg_slam_amd.datasets: {datapath}/results holds {n_img} frame*.jpg and {len(depth_paths)} "
                                "depth*.png")
    timestamps = [i / 30.0 for i in range(n_img)]
    with open(f"{datapath}/traj.txt", "r") as f:
        lines = f.readlines()
    poses, pose_w_t0 = [], np.eye(4)
    for i in range(n_img):
        c2w = np.array(list(map(float, lines[i].split()))).reshape(4, 4)
        if i == 0:
            pose_w_t0 = np.linalg.inv(c2w)
        poses.append(pose_w_t0 @ c2w)
    if frame_num != -1:
        frame_num = min(n_img, frame_num)
    indices = _select(n_img, frame_start, frame_num, frame_step)
    with open(os.path.join(datapath, "../cam_params.json"), "r") as f:
        cfg = json.load(f)["camera"]
    K = np.eye(3)
    K[0, 0] = cfg["fx"]
    K[1, 1] = cfg["fx"]
    K[0, 2] = cfg["cx"]
    K[1, 2] = cfg["cy"]
    scene = os.path.basename(os.path.normpath(datapath))
    return read_cameras("Replica", datapath, color_paths, depth_paths, poses, K, indices, cfg["scale"], timestamps, 0,
                        os.path.join(datapath, f"{scene}.ply"))


def _parse_list(path: str, skiprows: int = 0) -> np.ndarray:
    """np.loadtxt(path, delimiter=" ", dtype=str, skiprows=skiprows): the first `skiprows` lines go whatever they hold,
    then `#` comment lines and blank lines are skipped."""
    with open(path, "r") as f:
        lines = f.read().splitlines()[skiprows:]
    rows = []
    for ln in lines:
        ln = ln.split("#", 1)[0].strip()
        if ln:
            rows.append(ln.split(" "))
    return np.array(rows, dtype=str)


def quat_to_matrix(q) -> np.ndarray:
    """scipy.spatial.transform.Rotation.from_quat(q).as_matrix() for one scalar-last quaternion (x, y, z, w), normalised."""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(np.asarray(q, dtype=np.float64))
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return np.array([[x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)],
                     [2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)],
                     [2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2]])


def read_tum(datapath: str, frame_start: int = 0, frame_num: int = -1, frame_step: int = 0) -> DatasetInfo:
    """readTumSceneInfo (:545-690).  Each colour frame is paired with the nearest depth and pose timestamps, kept when both
    are within max_dt = 0.08 s.  The 32 fps rule then walks the pairs and keeps one when it comes more than 1/32 s after
    the last kept one - and, as in the reference (:619-630), only the NUMBER of kept pairs survives: the frame selection
    (frame_start + i * (frame_step + 1), bounded by that number) indexes the associated pairs themselves.  Poses are
    scalar-last quaternions (groundtruth.txt or pose.txt, first line skipped), made relative to the first selected frame;
    the frames are stably sorted by image name (the colour file's basename up to its first dot), as the reference sorts
    its cameras (:648)."""
    import yaml
    if os.path.isfile(os.path.join(datapath, "groundtruth.txt")):
        pose_list = os.path.join(datapath, "groundtruth.txt")
    elif os.path.isfile(os.path.join(datapath, "pose.txt")):
        pose_list = os.path.join(datapath, "pose.txt")
    else:
        raise FileNotFoundError(f"rtg_slam_amd.datasets: {datapath} has neither groundtruth.txt nor pose.txt")
    with open(os.path.join(datapath, "config.yaml"), "r") as f:
        cfg = yaml.safe_load(f)
    K = np.array([[cfg["fx"], 0, cfg["cx"]], [0, cfg["fy"], cfg["cy"]], [0, 0, 1]], dtype=np.float64)
    image_data = _parse_list(os.path.join(datapath, "rgb.txt"))
    depth_data = _parse_list(os.path.join(datapath, "depth.txt"))
    pose_data = _parse_list(pose_list, skiprows=1)
    pose_vecs = pose_data[:, 1:].astype(np.float64)
    t_img = image_data[:, 0].astype(np.float64)
    t_depth = depth_data[:, 0].astype(np.float64)
    t_pose = pose_data[:, 0].astype(np.float64)
    max_dt = 0.08
    assoc = []
    for i, t in enumerate(t_img):
        j = int(np.argmin(np.abs(t_depth - t)))
        k = int(np.argmin(np.abs(t_pose - t)))
        if np.abs(t_depth[j] - t) < max_dt and np.abs(t_pose[k] - t) < max_dt:
            assoc.append((i, j, k))
    kept = [0]
    for i in range(1, len(assoc)):
        if t_img[assoc[i][0]] - t_img[assoc[kept[-1]][0]] > 1.0 / 32:
            kept.append(i)
    n_img = len(kept) if assoc else 0
    sel = _select(n_img, frame_start, frame_num, frame_step)
    color_paths, depth_paths, poses, stamps = [], [], [], []
    inv_pose = None
    for ix in sel:
        i, j, k = assoc[ix]
        color_paths.append(os.path.join(datapath, image_data[i, 1]))
        depth_paths.append(os.path.join(datapath, depth_data[j, 1]))
        T = np.eye(4)
        T[:3, :3] = quat_to_matrix(pose_vecs[k][3:])
        T[:3, 3] = pose_vecs[k][:3]
        if inv_pose is None:
            inv_pose = np.linalg.inv(T)
            T = np.eye(4)
        else:
            T = inv_pose @ T
        poses.append(T)
        stamps.append(t_img[i])
    info = read_cameras("TUM", datapath, color_paths, depth_paths, poses, K, range(len(color_paths)), cfg["depth_scale"],
                        stamps, int(cfg["crop_edge"]), None)
    info.frames = sorted(info.frames, key=lambda fr: fr.image_name)
    return info


def read_ours(datapath: str, frame_start: int = 0, frame_num: int = -1, frame_step: int = 0, scannetpp: bool = False) -> DatasetInfo:
    """readOursSceneInfo (:968-1074) without its eval branch: color/*.jpg, depth/*.png, pose/*.txt each sorted by the
    integer value of the file name; intrinsics from intrinsic/intrinsic_depth.txt; depth scale 1000; no crop."""
    key = lambda p: int(os.path.basename(p).split(".")[0])
    color_paths = sorted(glob.glob(f"{datapath}/color/*.jpg"), key=key)
    depth_paths = sorted(glob.glob(f"{datapath}/depth/*.png"), key=key)
    pose_paths = sorted(glob.glob(f"{datapath}/pose/*.txt"), key=key)
    n_img = len(color_paths)
    if n_img == 0 or len(depth_paths) < n_img or len(pose_paths) < n_img:
        raise FileNotFoundError(f"rtg_slam_amd.datasets: {datapath} holds {n_img} colour, {len(depth_paths)} depth and "
                                f"{len(pose_paths)} pose files")
    timestamps = [(i + 1) / 30.0 for i in range(n_img)]
    poses = [np.loadtxt(pose_paths[i]) for i in range(n_img)]
    indices = _select(n_img, frame_start, frame_num, frame_step)
    K = np.loadtxt(os.path.join(datapath, "intrinsic", "intrinsic_depth.txt"))
    mesh = os.path.join(datapath, "mesh_aligned_cull.ply") if scannetpp else None
    return read_cameras("Scannetpp" if scannetpp else "Ours", datapath, color_paths, depth_paths, poses, K, indices, 1000.0,
                        timestamps, 0, mesh)


def loadcam_size(width: int, height: int, resolution, resolution_scale: float = 1.0):
    """The (w, h) utils/camera_utils.py:22-47 (loadCam) resizes a width x height frame to."""
    if resolution in [1, 2, 4, 8]:
        return (round(width / (resolution_scale * resolution)), round(height / (resolution_scale * resolution)))
    if resolution == -1:
        global_down = width / 1600 if width > 1600 else 1
    else:
        global_down = width / resolution
    scale = float(global_down) * float(resolution_scale)
    return (int(width / scale), int(height / scale))


def resized_intrinsics(fx: float, fy: float, cx: float, cy: float, width: int, height: int, out_width: int, out_height: int,
                       resolution_scale: float):
    """The intrinsics the reference gives a width x height camera whose frames loadCam resizes to out_width x out_height:
    the focal lengths go through the field of view of the cropped image (readCameras :908-909 focal2fov, scene/cameras.py
    fov2focal at the new size), cx and cy are divided by resolution_scale (camera_utils.py:69-70)."""
    fov_x = 2 * math.atan(width / (2 * fx))
    fov_y = 2 * math.atan(height / (2 * fy))
    return (out_width / (2 * math.tan(fov_x / 2)), out_height / (2 * math.tan(fov_y / 2)),
            cx / resolution_scale, cy / resolution_scale)


def resize_info(info: DatasetInfo, resolution_scale: float, resolution=1) -> DatasetInfo:
    """`info` (at its cropped size) with loadCam's resize by `resolution_scale` applied: output size and intrinsics.
    `resolution` must be one that by itself keeps the size; it only selects loadCam's rounding (round() for 1, int() for
    -1 or the frame width).  Scale 1 returns `info` itself."""
    s = float(resolution_scale)
    if not s > 0 or info.resized:
        raise ValueError(f"rtg_slam_amd.datasets: resolution scale {resolution_scale!r} (> 0 expected, on an unresized dataset)")
    W, H = info.crop_width, info.crop_height
    Wo, Ho = loadcam_size(W, H, resolution, s)
    if Wo <= 0 or Ho <= 0:
        raise ValueError(f"rtg_slam_amd.datasets: resolution scale {s} leaves nothing of the {W}x{H} frames")
    if (Wo, Ho) == (W, H) and s == 1.0:
        return info
    fx, fy, cx, cy = resized_intrinsics(info.fx, info.fy, info.cx, info.cy, W, H, Wo, Ho, s)
    return dataclasses.replace(info, fx=fx, fy=fy, cx=cx, cy=cy, resolution_scale=s, out_width=int(Wo), out_height=int(Ho))


def load_dataset(args) -> DatasetInfo:
    """The reader of args.type over args.source_path with args.frame_start / frame_num / frame_step (scene/__init__.py:25-68).
    args.resolution_scales[0] > 0 is loadCam's resolution_scale: the frames are resized on the device and the intrinsics
    follow (resize_info).  Rejects eval: true, and any `resolution` that by itself would make loadCam resize the frames."""
    if bool(getattr(args, "eval", False)):
        raise ValueError("rtg_slam_amd.datasets: `eval: true` (train / test frame split) is not supported; no shipped config "
                         "sets it, and the reference's own eval path of the Ours reader is broken")
    typ = getattr(args, "type", "Replica")
    sel = dict(frame_start=int(getattr(args, "frame_start", 0)), frame_num=int(getattr(args, "frame_num", -1)),
               frame_step=int(getattr(args, "frame_step", 0)))
    src = args.source_path
    if typ == "Replica":
        info = read_replica(src, **sel)
    elif typ == "TUM":
        info = read_tum(src, **sel)
    elif typ in ("Ours", "Scannetpp"):
        info = read_ours(src, scannetpp=(typ == "Scannetpp"), **sel)
    else:
        raise ValueError(f"rtg_slam_amd.datasets: unknown dataset type {typ!r}")
    scales = list(getattr(args, "resolution_scales", [1.0]) or [1.0])
    resolution = getattr(args, "resolution", 1)
    want = loadcam_size(info.width, info.height, resolution, 1.0)
    if tuple(want) != (info.width, info.height):
        raise ValueError(f"rtg_slam_amd.datasets: resolution {resolution} would resize the {info.width}x{info.height} frames "
                         f"to {want[0]}x{want[1]}, and the reference divides cx, cy by resolution_scale only, never by "
                         "`resolution`: the resized camera would be wrong.  Use resolution_scales: [S] (or "
                         "--resolution-scale S) to run at a reduced size")
    if not float(scales[0]) > 0:
        raise ValueError(f"rtg_slam_amd.datasets: resolution_scales {scales}: the first entry must be > 0")
    return resize_info(info, float(scales[0]), resolution)


def read_pose_t0(args) -> np.ndarray:
    """metric.py:77-88: the dataset's first raw pose (the reconstruction's transform to the GT mesh's frame)."""
    if args.type == "Replica":
        return np.loadtxt(os.path.join(args.source_path, "traj.txt"))[0].reshape(4, 4)
    if args.type == "Scannetpp":
        return np.loadtxt(os.path.join(args.source_path, "pose", "0000.txt")).reshape(4, 4)
    return np.eye(4)


# ---------------------------------------------------------------------------------------------------------------- decode
def decode_depth(path: str) -> np.ndarray:
    """The depth PNG as u16 [H,W].  Pillow opens 16-bit PNGs as `I;16` (uint16); older versions give `I` (int32): both are
    accepted, values outside 0..65535 are rejected."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.ndim != 2 or a.dtype.kind not in "ui" or a.dtype.itemsize > 4:
        raise ValueError(f"rtg_slam_amd.datasets: {path}: depth must be a single-channel integer image, got {a.dtype} {a.shape}")
    if a.dtype.itemsize > 2 or a.dtype.kind == "i":
        if a.size and (int(a.min()) < 0 or int(a.max()) > 65535):
            raise ValueError(f"rtg_slam_amd.datasets: {path}: depth values outside 0..65535")
    return a.astype(np.uint16, copy=False)


def decode_color(path: str, width: int, height: int) -> np.ndarray:
    """The colour image as u8 [H,W,3|4], resized to the depth's size with PIL's default filter when the sizes differ
    (readCameras :893-895)."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA"):
            raise ValueError(f"rtg_slam_amd.datasets: {path}: colour mode {im.mode} (RGB or RGBA expected)")
        if im.size != (width, height):
            im = im.resize((width, height))
        a = np.asarray(im)
    return a


def reference_chain(depth_u16: np.ndarray, color_u8: np.ndarray, depth_scale: float, crop: int):
    """The reference's float chain on the CPU (numpy float32 scaling, PILtoTorch's / 255 in torch), cropped: -> (depth [H,W]
    after / 255, colour [3,H,W]); the loop multiplies the depth by 255 on the device.  For tests and tools."""
    d = np.asarray(depth_u16, dtype=np.float32) / depth_scale
    c = np.array(color_u8)
    if crop > 0:
        d = d[crop:-crop, crop:-crop]
        c = c[crop:-crop, crop:-crop, :]
    d_t = torch.from_numpy(np.ascontiguousarray(d)) / 255.0
    c_t = (torch.from_numpy(np.ascontiguousarray(c)) / 255.0).permute(2, 0, 1)[:3]
    return d_t, c_t


# ---------------------------------------------------------------------------------------------------------------- resize
RESAMPLE_BITS = 22                        # Pillow's 8-bit resampler: coefficients in fixed point with 32 - 8 - 2 fractional bits


def resample_tables(in_size: int, out_size: int):
    """Pillow's BILINEAR coefficients for resampling one axis of in_size pixels to out_size (its precompute_coeffs and
    normalize_coeffs_8bpc), in float64 as Pillow computes them in C doubles: -> (start int32 [out], length int32 [out],
    coeff int32 [out, ksize]).  Output index i is sum(coeff[i, :length[i]] * src[start[i] : start[i] + length[i]]); the
    triangle filter's support is widened by the reduction factor (1 when enlarging), the weights are normalised to sum 1,
    then rounded to RESAMPLE_BITS fractional bits; coeff is zero beyond length."""
    n_in, n_out = int(in_size), int(out_size)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"rtg_slam_amd.datasets: resample_tables({in_size}, {out_size}): sizes must be positive")
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    ss = 1.0 / filterscale
    start = (center - support + 0.5).astype(np.int64)              # C's (int): truncation
    start[start < 0] = 0
    stop = (center + support + 0.5).astype(np.int64)
    stop[stop > n_in] = n_in
    length = stop - start
    k = np.zeros((n_out, ksize), dtype=np.float64)
    ww = np.zeros(n_out, dtype=np.float64)
    for x in range(ksize):                                         # ww accumulates in x order, as the C loop does
        w = np.abs(((x + start).astype(np.float64) - center + 0.5) * ss)
        w = np.where((w < 1.0) & (x < length), 1.0 - w, 0.0)
        k[:, x] = w
        ww = ww + w
    nz = ww != 0.0
    k[nz] = k[nz] / ww[nz, None]
    coeff = (0.5 + k * float(1 << RESAMPLE_BITS)).astype(np.int64)  # the bilinear weights are never negative
    coeff[np.arange(ksize)[None, :] >= length[:, None]] = 0
    return start.astype(np.int32), length.astype(np.int32), np.ascontiguousarray(coeff.astype(np.int32))


def nearest_indices(in_size: int, out_size: int) -> np.ndarray:
    """The source index Pillow's NEAREST resize picks for every output index (its affine scaling walks the source coordinate
    by repeated addition in a C double, starting half a step in): int32 [out]."""
    n_in, n_out = int(in_size), int(out_size)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"rtg_slam_amd.datasets: nearest_indices({in_size}, {out_size}): sizes must be positive")
    step = n_in / n_out
    pos = np.empty(n_out, dtype=np.float64)
    xo = step * 0.5
    for i in range(n_out):
        pos[i] = xo
        xo += step
    return np.clip(pos.astype(np.int64), 0, n_in - 1).astype(np.int32)


def _resample_axis0(a: np.ndarray, tables) -> np.ndarray:
    start, length, coeff = tables
    acc = np.full((len(start),) + a.shape[1:], 1 << (RESAMPLE_BITS - 1), dtype=np.int64)
    src = a.astype(np.int64)
    for j in range(coeff.shape[1]):
        idx = np.minimum(start.astype(np.int64) + j, a.shape[0] - 1)          # beyond `length` the coefficient is 0
        acc += coeff[:, j].astype(np.int64).reshape((-1,) + (1,) * (a.ndim - 1)) * src[idx]
    return np.clip(acc >> RESAMPLE_BITS, 0, 255).astype(np.uint8)


def reference_resize(color_u8: np.ndarray, depth_f32, out_w: int, out_h: int):
    """PIL's `resize((out_w, out_h), BILINEAR)` of a u8 [H,W,3|4] image and `resize((out_w, out_h), NEAREST)` of a [H,W] depth
    image (either may be None), in numpy through resample_tables / nearest_indices: the arithmetic of
    rtgs_ingest_rgbd_resized.  Colour: a horizontal pass, then a vertical pass on the rounded u8 result of the first; an
    RGBA image is resampled with its colours premultiplied by alpha and divided by the resampled alpha afterwards, as
    Image.resize does (modes RGBa / RGBA).  An image that already has the size is returned as it is."""
    color = depth = None
    if color_u8 is not None:
        a = np.asarray(color_u8)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
            raise ValueError("rtg_slam_amd.datasets.reference_resize: colour u8 [H,W,3|4] expected")
        if (a.shape[1], a.shape[0]) == (out_w, out_h):
            color = a.copy()
        else:
            if a.shape[2] == 4:
                t = a[..., :3].astype(np.int64) * a[..., 3:4].astype(np.int64) + 128
                a = np.concatenate([(((t >> 8) + t) >> 8).astype(np.uint8), a[..., 3:4]], axis=2)
            h = _resample_axis0(a.transpose(1, 0, 2), resample_tables(a.shape[1], out_w)).transpose(1, 0, 2)
            color = _resample_axis0(h, resample_tables(a.shape[0], out_h))
            if color.shape[2] == 4:
                al = color[..., 3:4].astype(np.int64)
                un = np.minimum(255 * color[..., :3].astype(np.int64) // np.maximum(al, 1), 255)
                color[..., :3] = np.where((al == 0) | (al == 255), color[..., :3], un).astype(np.uint8)
    if depth_f32 is not None:
        d = np.asarray(depth_f32)
        if d.ndim != 2:
            raise ValueError("rtg_slam_amd.datasets.reference_resize: depth [H,W] expected")
        depth = d.copy() if (d.shape[1], d.shape[0]) == (out_w, out_h) else \
            d[nearest_indices(d.shape[0], out_h)[:, None], nearest_indices(d.shape[1], out_w)[None, :]]
    return color, depth


# ---------------------------------------------------------------------------------------------------------------- ingest
@dataclass
class ResizeTables:
    """What rtgs_ingest_rgbd_resized reads per (cropped size, output size): the packed int32 buffer of include/rtgs_slam.h
    (x_start x_len x_near y_start y_len y_near x_coeff y_coeff), on the host (`packed`) and, after to(), on a device."""
    in_size: tuple                        # (W, H) after the crop
    out_size: tuple                       # (Wo, Ho)
    x_ksize: int
    y_ksize: int
    packed: np.ndarray
    device_buf: Optional[torch.Tensor] = None

    def expected_len(self) -> int:
        Wo, Ho = self.out_size
        return 3 * Wo + 3 * Ho + Wo * self.x_ksize + Ho * self.y_ksize

    def to(self, device) -> "ResizeTables":
        return dataclasses.replace(self, device_buf=torch.from_numpy(self.packed).to(device))


def resize_tables(in_size, out_size) -> ResizeTables:
    """The tables of resample_tables / nearest_indices for resizing (W, H) frames to (Wo, Ho), packed for the kernel."""
    (W, H), (Wo, Ho) = (int(v) for v in in_size), (int(v) for v in out_size)
    xs, xl, xk = resample_tables(W, Wo)
    ys, yl, yk = resample_tables(H, Ho)
    packed = np.concatenate([xs, xl, nearest_indices(W, Wo), ys, yl, nearest_indices(H, Ho), xk.reshape(-1),
                             yk.reshape(-1)]).astype(np.int32)
    return ResizeTables((W, H), (Wo, Ho), int(xk.shape[1]), int(yk.shape[1]), np.ascontiguousarray(packed))


def ingest(depth_raw: torch.Tensor, color_raw: torch.Tensor, depth_scale: float, crop: int = 0, stream=None, out_size=None,
           tables: Optional[ResizeTables] = None):
    """rtgs_ingest_rgbd on the device: depth_raw u16 [Hd,Wd] (int16 / uint16 storage), color_raw u8 [Hd,Wd,3|4] ->
    (depth [H,W,1] metres, colour [3,H,W]) float32, enqueued on `stream` (default: the current stream).  With an
    `out_size` (Wo, Ho) other than the cropped size, rtgs_ingest_rgbd_resized: the frame resized after the crop as loadCam
    does with PIL, -> (depth [Ho,Wo,1], colour [3,Ho,Wo]); `tables` (resize_tables(...).to(device), built for these very
    sizes) spares computing and uploading them per call."""
    from . import _lib
    if not (depth_raw.is_cuda and color_raw.is_cuda):
        raise RuntimeError("rtg_slam_amd.datasets.ingest: tensors must live on a HIP device; this build has no CPU path.")
    if depth_raw.dim() != 2 or depth_raw.element_size() != 2 or color_raw.dtype != torch.uint8 or color_raw.dim() != 3 \
            or tuple(color_raw.shape[:2]) != tuple(depth_raw.shape) or color_raw.shape[2] not in (3, 4):
        raise ValueError("rtg_slam_amd.datasets.ingest: depth u16 [Hd,Wd] and colour u8 [Hd,Wd,3|4] expected")
    Hd, Wd, ch = int(depth_raw.shape[0]), int(depth_raw.shape[1]), int(color_raw.shape[2])
    H, W = Hd - 2 * crop, Wd - 2 * crop
    if crop < 0 or H <= 0 or W <= 0:
        raise ValueError(f"rtg_slam_amd.datasets.ingest: crop {crop} does not fit {Hd}x{Wd}")
    dev = depth_raw.device
    resized = False
    if out_size is not None:
        Wo, Ho = int(out_size[0]), int(out_size[1])
        if Wo <= 0 or Ho <= 0:
            raise ValueError(f"rtg_slam_amd.datasets.ingest: out_size {tuple(out_size)} must be positive")
        resized = (Wo, Ho) != (W, H)
    if resized:
        if tables is None:
            tables = resize_tables((W, H), (Wo, Ho))
        if tuple(tables.in_size) != (W, H) or tuple(tables.out_size) != (Wo, Ho):
            raise ValueError(f"rtg_slam_amd.datasets.ingest: tables for {tables.in_size} -> {tables.out_size}, frame "
                             f"{(W, H)} -> {(Wo, Ho)}")
        if tables.device_buf is None or tables.device_buf.device != dev:
            tables = tables.to(dev)
        buf = tables.device_buf
        if buf.dtype != torch.int32 or buf.dim() != 1 or not buf.is_contiguous() or buf.numel() != tables.expected_len():
            raise ValueError(f"rtg_slam_amd.datasets.ingest: resize tables must be {tables.expected_len()} contiguous int32 "
                             f"values, got {buf.dtype} {tuple(buf.shape)}")
    else:
        Wo, Ho = W, H
    st = torch.cuda.current_stream(dev) if stream is None else stream
    dr, cr = depth_raw.contiguous(), color_raw.contiguous()
    with torch.cuda.stream(st):
        depth = torch.empty(Ho, Wo, 1, dtype=torch.float32, device=dev)
        color = torch.empty(3, Ho, Wo, dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        if resized:
            rc = lib.rtgs_ingest_rgbd_resized(C.c_void_p(dr.data_ptr()), C.c_void_p(cr.data_ptr()), Hd, Wd, ch, int(crop),
                                              float(depth_scale), Ho, Wo, C.c_void_p(buf.data_ptr()), int(buf.numel()),
                                              int(tables.x_ksize), int(tables.y_ksize), C.c_void_p(depth.data_ptr()),
                                              C.c_void_p(color.data_ptr()), C.c_void_p(st.cuda_stream))
            if stream is not None:
                buf.record_stream(st)
        else:
            rc = lib.rtgs_ingest_rgbd(C.c_void_p(dr.data_ptr()), C.c_void_p(cr.data_ptr()), Hd, Wd, ch, int(crop),
                                      float(depth_scale), C.c_void_p(depth.data_ptr()), C.c_void_p(color.data_ptr()),
                                      C.c_void_p(st.cuda_stream))
    _lib.check(rc, "rtgs_ingest_rgbd_resized" if resized else "rtgs_ingest_rgbd")
    return depth, color


def default_io_workers() -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:                                         # pragma: no cover - not Linux
        n = os.cpu_count() or 1
    return max(1, min(8, n, MAX_IO_WORKERS))


class _Slot:
    """One staging slot: pinned host bytes for a frame's raw depth and colour, the device copy of them, and the event after
    the host-to-device copy of the frame that used the slot last."""

    def __init__(self, n_pix: int, device):
        self.host_depth = torch.empty(n_pix, dtype=torch.int16, pin_memory=True)
        self.host_color = torch.empty(n_pix * 4, dtype=torch.uint8, pin_memory=True)
        self.dev_depth = torch.empty(n_pix, dtype=torch.int16, device=device)
        self.dev_color = torch.empty(n_pix * 4, dtype=torch.uint8, device=device)
        self.copied: Optional[torch.cuda.Event] = None


class FrameSource:
    """Streams a `DatasetInfo`'s frames to `device` as (depth [H,W,1], colour [3,H,W], c2w float64 [4,4]), H x W the
    info's output size (the resize of a resized info happens in the ingest launch; the bytes copied per frame stay the raw
    frame's).

    io_workers decode threads (default min(8, CPUs this process may use), at most 16); `prefetch` frames in flight at most
    (default io_workers + 2), one pinned staging slot each.  A worker decodes frame i, waits until the copy of the frame
    that used its slot before has completed, writes the raw bytes into the slot and at once enqueues, on the source's own
    stream, the copy to the device, the ingest kernel and an event.  next() waits for frame i's worker (that wait is
    counted in `io_wait_s`), makes the consumer's current stream wait on the event, marks the tensors as used on that
    stream (record_stream) and hands frame i + prefetch to the pool.  prefetch = 1 with one worker runs the same code.
    Statistics of the last pass: frames, io_wait_s, decode_s (summed over the workers), h2d_bytes; and the output size."""

    def __init__(self, info: DatasetInfo, device, io_workers: Optional[int] = None, prefetch: Optional[int] = None):
        self.info = info
        self.device = torch.device(device)
        w = default_io_workers() if io_workers is None else int(io_workers)
        if not 1 <= w <= MAX_IO_WORKERS:
            raise ValueError(f"rtg_slam_amd.datasets: io_workers must be 1..{MAX_IO_WORKERS}, got {w}")
        self.io_workers = w
        self.prefetch = max(1, int(prefetch) if prefetch is not None else w + 2)
        self.frames = 0
        self.io_wait_s = 0.0
        self.decode_s = 0.0
        self.h2d_bytes = 0
        self._lock = threading.Lock()
        self._stream = None
        self._slots: List[_Slot] = []
        self._tables: Optional[ResizeTables] = None

    def __len__(self) -> int:
        return len(self.info.frames)

    def _ensure(self):
        if self._stream is None:
            self._stream = torch.cuda.Stream(self.device)
            n_pix = self.info.raw_height * self.info.raw_width
            self._slots = [_Slot(n_pix, self.device) for _ in range(self.prefetch)]
            if self.info.resized:                           # computed and uploaded once; every frame's launch reads them
                self._tables = resize_tables((self.info.crop_width, self.info.crop_height),
                                             (self.info.width, self.info.height)).to(self.device)

    def _work(self, i: int):
        info, rec = self.info, self.info.frames[i]
        slot = self._slots[i % self.prefetch]
        t0 = time.perf_counter()
        depth = decode_depth(rec.depth_path)
        if depth.shape != (info.raw_height, info.raw_width):
            raise ValueError(f"rtg_slam_amd.datasets: {rec.depth_path} is {depth.shape[1]}x{depth.shape[0]}, the dataset's "
                             f"frames are {info.raw_width}x{info.raw_height}")
        color = decode_color(rec.color_path, info.raw_width, info.raw_height)
        t1 = time.perf_counter()
        if slot.copied is not None:
            slot.copied.synchronize()                       # the slot's previous frame has left the pinned buffer
        n_pix, ch = depth.size, int(color.shape[2])
        np.copyto(slot.host_depth.numpy().view(np.uint16), depth.reshape(-1))
        np.copyto(slot.host_color[:n_pix * ch].numpy(), color.reshape(-1))
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            slot.dev_depth.copy_(slot.host_depth, non_blocking=True)
            slot.dev_color[:n_pix * ch].copy_(slot.host_color[:n_pix * ch], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(self._stream)
            slot.copied = copied
            d, c = ingest(slot.dev_depth.view(info.raw_height, info.raw_width),
                          slot.dev_color[:n_pix * ch].view(info.raw_height, info.raw_width, ch), info.depth_scale,
                          info.crop_edge, self._stream, out_size=(info.width, info.height), tables=self._tables)
            ready = torch.cuda.Event()
            ready.record(self._stream)
        with self._lock:
            self.decode_s += t1 - t0
            self.h2d_bytes += n_pix * (2 + ch)
        return d, c, rec.c2w.copy(), ready

    def __iter__(self):
        self._ensure()
        self.frames, self.io_wait_s, self.decode_s, self.h2d_bytes = 0, 0.0, 0.0, 0
        n = len(self.info.frames)
        pool = ThreadPoolExecutor(max_workers=self.io_workers, thread_name_prefix="rtgs-io")
        futures = {}
        try:
            for i in range(min(self.prefetch, n)):
                futures[i] = pool.submit(self._work, i)
            for i in range(n):
                t0 = time.perf_counter()
                d, c, c2w, ready = futures.pop(i).result()
                self.io_wait_s += time.perf_counter() - t0
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ready)
                d.record_stream(cur)
                c.record_stream(cur)
                # slot i % prefetch is free for frame i + prefetch once frame i's upload is enqueued, which it is
                if i + self.prefetch < n:
                    futures[i + self.prefetch] = pool.submit(self._work, i + self.prefetch)
                self.frames += 1
                yield d, c, c2w
        finally:
            for f in futures.values():
                f.cancel()
            pool.shutdown(wait=True)

    def stats(self) -> dict:
        n = max(self.frames, 1)
        return {"frames": self.frames, "io_workers": self.io_workers, "prefetch": self.prefetch,
                "io_wait_s": self.io_wait_s, "io_wait_s_mean": self.io_wait_s / n,
                "decode_ms_per_frame": 1e3 * self.decode_s / n, "h2d_bytes_per_frame": self.h2d_bytes / n,
                "width": self.info.width, "height": self.info.height, "resolution_scale": self.info.resolution_scale}
