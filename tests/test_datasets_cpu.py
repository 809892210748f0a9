"""rtg_slam_amd.datasets readers against a restatement of the reference's live reader paths (scene/dataset_readers.py:
readReplicaSceneInfo :774-846, readTumSceneInfo :545-690, readOursSceneInfo :968-1074, all ending in readCameras :848-932)
on tiny datasets written here with PIL: frame lists, intrinsics, poses and the decoded raw arrays."""
import glob
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from rtg_slam_amd import datasets as ds


# ------------------------------------------------------------------------------------------------ restated reference
def _ref_read_cameras(color_paths, depth_paths, poses, intrinsic, indices, depth_scale, crop_edge=0):
    """readCameras, decoding included (what the reference's loop gets, before PILtoTorch)."""
    poses = [np.array(p, dtype=np.float64) for p in poses]
    out = []
    pose_w_t0 = np.eye(4)
    for idx_ in range(len(indices)):
        idx = indices[idx_]
        c2w = poses[idx]
        if idx_ == 0:
            pose_w_t0 = np.linalg.inv(c2w)
        if np.isinf(c2w).any():
            continue
        c2w = pose_w_t0 @ c2w
        poses[idx] = c2w
        image_color = Image.open(color_paths[idx])
        raw_depth = np.asarray(Image.open(depth_paths[idx]))
        image_depth = np.asarray(Image.open(depth_paths[idx]), dtype=np.float32) / depth_scale
        image_color = np.asarray(image_color.resize((image_depth.shape[1], image_depth.shape[0])))
        fx, fy, cx, cy = intrinsic[0, 0], intrinsic[1, 1], intrinsic[0, 2], intrinsic[1, 2]
        if crop_edge > 0:
            image_color = image_color[crop_edge:-crop_edge, crop_edge:-crop_edge, :]
            image_depth = image_depth[crop_edge:-crop_edge, crop_edge:-crop_edge]
            cx -= crop_edge
            cy -= crop_edge
        out.append(dict(color_path=color_paths[idx], depth_path=depth_paths[idx], c2w=c2w, fx=fx, fy=fy, cx=cx, cy=cy,
                        image_name=os.path.basename(color_paths[idx]).split(".")[0], color=image_color, depth=image_depth,
                        raw_depth=raw_depth))
    return out


def _ref_replica(datapath, frame_start, frame_num, frame_step):
    color_paths = sorted(glob.glob(f"{datapath}/results/frame*.jpg"))
    depth_paths = sorted(glob.glob(f"{datapath}/results/depth*.png"))
    n_img = len(color_paths)
    lines = open(f"{datapath}/traj.txt").readlines()
    poses = []
    for i in range(n_img):
        c2w = np.array(list(map(float, lines[i].split()))).reshape(4, 4)
        if i == 0:
            pose_w_t0 = np.linalg.inv(c2w)
        poses.append(pose_w_t0 @ c2w)
    indicies = list(range(n_img)) if frame_num == -1 else list(range(min(n_img, frame_num)))
    indicies = [frame_start + i * (frame_step + 1) for i in indicies]
    indicies = [i for i in indicies if i < n_img]                    # the bound this package adds
    config = json.load(open(os.path.join(datapath, "../cam_params.json")))["camera"]
    K = np.eye(3)
    K[0, 0] = K[1, 1] = config["fx"]
    K[0, 2], K[1, 2] = config["cx"], config["cy"]
    return _ref_read_cameras(color_paths, depth_paths, poses, K, indicies, config["scale"])


def _scipy_form_quat(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[x * x - y * y - z * z + w * w, 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), -x * x - y * y + z * z + w * w]])


def _ref_tum(datapath, frame_start, frame_num, frame_step):
    import yaml
    parse = lambda p, skiprows=0: np.loadtxt(p, delimiter=" ", dtype=str, skiprows=skiprows)
    pose_list = os.path.join(datapath, "groundtruth.txt")
    config = yaml.safe_load(open(os.path.join(datapath, "config.yaml")))
    K = np.array([[config["fx"], 0, config["cx"]], [0, config["fy"], config["cy"]], [0, 0, 1]])
    image_data, depth_data = parse(os.path.join(datapath, "rgb.txt")), parse(os.path.join(datapath, "depth.txt"))
    pose_data = parse(pose_list, skiprows=1)
    pose_vecs = pose_data[:, 1:].astype(np.float64)
    t_img, t_depth, t_pose = (a[:, 0].astype(np.float64) for a in (image_data, depth_data, pose_data))
    assoc = []
    for i, t in enumerate(t_img):
        j, k = np.argmin(np.abs(t_depth - t)), np.argmin(np.abs(t_pose - t))
        if np.abs(t_depth[j] - t) < 0.08 and np.abs(t_pose[k] - t) < 0.08:
            assoc.append((i, j, k))
    indicies = [0]
    for i in range(1, len(assoc)):
        if t_img[assoc[i][0]] - t_img[assoc[indicies[-1]][0]] > 1.0 / 32:
            indicies += [i]
    n_img = len(indicies)
    indexs = list(range(n_img)) if frame_num == -1 else list(range(frame_num))
    indicies = [frame_start + i * (frame_step + 1) for i in indexs]
    indicies = [i for i in indicies if i < n_img]
    color_paths, depth_paths, poses, inv_pose = [], [], [], None
    for ix in indicies:
        i, j, k = assoc[ix]
        color_paths.append(os.path.join(datapath, image_data[i, 1]))
        depth_paths.append(os.path.join(datapath, depth_data[j, 1]))
        c2w = np.eye(4)
        c2w[:3, :3] = _scipy_form_quat(pose_vecs[k][3:])
        c2w[:3, 3] = pose_vecs[k][:3]
        if inv_pose is None:
            inv_pose = np.linalg.inv(c2w)
            c2w = np.eye(4)
        else:
            c2w = inv_pose @ c2w
        poses.append(c2w)
    cams = _ref_read_cameras(color_paths, depth_paths, poses, K, range(len(color_paths)), config["depth_scale"],
                             config["crop_edge"])
    return sorted(cams, key=lambda c: c["image_name"]), assoc


def _ref_ours(datapath, frame_start, frame_num, frame_step):
    key = lambda x: int(os.path.basename(x).split(".")[0])
    color_paths = sorted(glob.glob(f"{datapath}/color/*.jpg"), key=key)
    depth_paths = sorted(glob.glob(f"{datapath}/depth/*.png"), key=key)
    pose_paths = sorted(glob.glob(f"{datapath}/pose/*.txt"), key=key)
    n_img = len(color_paths)
    poses = [np.loadtxt(pose_paths[i]) for i in range(n_img)]
    indicies = list(range(n_img)) if frame_num == -1 else list(range(frame_num))
    indicies = [frame_start + i * (frame_step + 1) for i in indicies]
    indicies = [i for i in indicies if i < n_img]
    K = np.loadtxt(os.path.join(datapath, "intrinsic", "intrinsic_depth.txt"))
    return _ref_read_cameras(color_paths, depth_paths, poses, K, indicies, 1000.0)


# ------------------------------------------------------------------------------------------------------- fixtures
def _pose(rng, scale=1.0):
    from rtg_slam_amd import synth
    import torch
    xi = torch.from_numpy(rng.normal(size=6) * np.array([0.3, 0.3, 0.3, scale, scale, scale]))
    return synth.se3_exp(xi).numpy()


def _write_frame(color_path, depth_path, rng, cw, ch, dw, dh, mode="RGB"):
    os.makedirs(os.path.dirname(color_path), exist_ok=True)
    os.makedirs(os.path.dirname(depth_path), exist_ok=True)
    c = rng.integers(0, 256, size=(ch, cw, 3 if mode == "RGB" else 4), dtype=np.uint8)
    Image.fromarray(c, mode).save(color_path, quality=90) if color_path.endswith(".jpg") else Image.fromarray(c, mode).save(color_path)
    d = rng.integers(0, 65536, size=(dh, dw), dtype=np.uint16)
    d[0, 0], d[-1, -1] = 0, 65535
    Image.fromarray(d).save(depth_path)


def _replica(root, n=6, first_pose_identity=False):
    rng = np.random.default_rng(1)
    scene = os.path.join(root, "Replica", "office0")
    lines = []
    for i in range(n):
        # colour 2x the depth: readCameras resizes it to the depth's size
        _write_frame(f"{scene}/results/frame{i:06d}.jpg", f"{scene}/results/depth{i:06d}.png", rng, 48, 32, 24, 16)
        P = np.eye(4) if (first_pose_identity and i == 0) else _pose(rng)
        lines.append(" ".join(repr(float(v)) for v in P.reshape(-1)))
    open(f"{scene}/traj.txt", "w").write("\n".join(lines) + "\n")
    json.dump({"camera": {"w": 24, "h": 16, "fx": 20.5, "fy": 21.75, "cx": 11.5, "cy": 7.25, "scale": 6553.5}},
              open(os.path.join(root, "Replica", "cam_params.json"), "w"))
    return scene


def _check_same(info, ref, crop=0):
    assert [f.color_path for f in info.frames] == [r["color_path"] for r in ref]
    assert [f.depth_path for f in info.frames] == [r["depth_path"] for r in ref]
    assert [f.image_name for f in info.frames] == [r["image_name"] for r in ref]
    for f, r in zip(info.frames, ref):
        np.testing.assert_allclose(f.c2w, r["c2w"], rtol=0, atol=1e-12)
        assert (info.fx, info.fy, info.cx, info.cy) == (r["fx"], r["fy"], r["cx"], r["cy"])
        raw = ds.decode_depth(f.depth_path)
        assert raw.dtype == np.uint16 and np.array_equal(raw, r["raw_depth"])
        col = ds.decode_color(f.color_path, info.raw_width, info.raw_height)
        d_t, c_t = ds.reference_chain(raw, col, info.depth_scale, crop)
        assert np.array_equal(d_t.numpy(), (__import__("torch").from_numpy(r["depth"]) / 255.0).numpy())
        assert np.array_equal(c_t.permute(1, 2, 0).mul(255).round().byte().numpy(), r["color"][..., :3])
        assert (info.height, info.width) == r["depth"].shape == r["color"].shape[:2]


# ---------------------------------------------------------------------------------------------------------- tests
def test_replica_poses_fy_selection_and_resize(tmp_path):
    scene = _replica(str(tmp_path))
    info = ds.read_replica(scene, frame_start=1, frame_num=5, frame_step=1)       # 1, 3, 5, 7, 9: past the end at 7
    ref = _ref_replica(scene, 1, 5, 1)
    assert len(info) == len(ref) == 3
    _check_same(info, ref)
    assert info.fx == info.fy == 20.5                                             # fy := fx
    assert info.depth_scale == 6553.5 and (info.raw_width, info.raw_height) == (24, 16)
    np.testing.assert_allclose(info.frames[0].c2w, np.eye(4), atol=1e-12)         # relative to the first SELECTED frame
    raw0 = np.loadtxt(f"{scene}/traj.txt")
    assert not np.allclose(raw0[0].reshape(4, 4), np.eye(4))                      # the first pose of traj.txt is not identity
    assert info.mesh_path == os.path.join(scene, "office0.ply")
    all_ = ds.read_replica(scene)
    assert len(all_) == 6 and [f.image_name for f in all_.frames] == [f"frame{i:06d}" for i in range(6)]
    _check_same(all_, _ref_replica(scene, 0, -1, 0))
    p0 = ds.read_pose_t0(SimpleNamespace(type="Replica", source_path=scene))
    np.testing.assert_array_equal(p0, raw0[0].reshape(4, 4))


def _tum(root):
    rng = np.random.default_rng(2)
    d = os.path.join(root, "tum")
    t_img = [1.00, 1.05, 1.06, 1.10, 1.30, 1.40, 1.50, 1.60]
    t_dep = [1.001, 1.049, 1.061, 1.102, 1.402, 1.499, 1.601]      # nothing near 1.30: dropped by the 0.08 s association
    t_pose = [0.99 + 0.01 * i for i in range(70)]
    rgb, dep = ["# colour images", "# file: x", "# timestamp filename"], ["# depth maps", "# x", "# timestamp filename"]
    for t in t_img:
        name = f"rgb/{t:.6f}.png"
        c = rng.integers(0, 256, size=(32, 40, 3), dtype=np.uint8)
        os.makedirs(os.path.join(d, "rgb"), exist_ok=True)
        Image.fromarray(c).save(os.path.join(d, name))
        rgb.append(f"{t:.6f} {name}")
    for t in t_dep:
        name = f"depth/{t:.6f}.png"
        os.makedirs(os.path.join(d, "depth"), exist_ok=True)
        Image.fromarray(rng.integers(0, 65536, size=(32, 40), dtype=np.uint16)).save(os.path.join(d, name))
        dep.append(f"{t:.6f} {name}")
    gt = ["# ground truth trajectory", "# file: x", "# timestamp tx ty tz qx qy qz qw"]
    for t in t_pose:
        q = rng.normal(size=4)
        tr = rng.normal(size=3)
        gt.append(" ".join([f"{t:.4f}"] + [f"{v:.6f}" for v in tr] + [f"{v:.6f}" for v in q]))
    for name, lines in (("rgb.txt", rgb), ("depth.txt", dep), ("groundtruth.txt", gt)):
        open(os.path.join(d, name), "w").write("\n".join(lines) + "\n")
    open(os.path.join(d, "config.yaml"), "w").write("fx: 30.0\nfy: 31.0\ncx: 19.5\ncy: 15.5\ndepth_scale: 5000.0\ncrop_edge: 8\n")
    return d


def test_tum_association_rate_rule_quaternions_and_crop(tmp_path):
    d = _tum(str(tmp_path))
    info = ds.read_tum(d)
    ref, assoc = _ref_tum(d, 0, -1, 0)
    assert len(assoc) == 7                                           # 1.30 has no depth within 0.08 s
    assert len(info) == len(ref) == 6                                # 1.06 is within 1/32 s of 1.05: one frame fewer
    _check_same(info, ref, crop=8)
    assert (info.cx, info.cy) == (19.5 - 8, 15.5 - 8) and (info.width, info.height) == (24, 16)
    assert info.depth_scale == 5000.0 and info.crop_edge == 8
    np.testing.assert_allclose(info.frames[0].c2w, np.eye(4), atol=1e-12)
    sub = ds.read_tum(d, frame_start=1, frame_num=10, frame_step=1)
    _check_same(sub, _ref_tum(d, 1, 10, 1)[0], crop=8)
    try:                                                             # the quaternion convention, where scipy is present
        from scipy.spatial.transform import Rotation
    except ImportError:
        Rotation = None
    q = np.array([0.3, -0.2, 0.5, 0.7])
    want = Rotation.from_quat(q).as_matrix() if Rotation is not None else _scipy_form_quat(q)
    np.testing.assert_allclose(ds.quat_to_matrix(q), want, rtol=0, atol=1e-15)


def test_tum_sorts_by_name_stably(tmp_path):
    d = _tum(str(tmp_path))
    # timestamps split at the first dot: "1" for every frame -> the stable sort keeps the association order
    info = ds.read_tum(d)
    assert [f.image_name for f in info.frames] == ["1"] * len(info)
    assert [f.timestamp for f in info.frames] == sorted(f.timestamp for f in info.frames)


def _ours(root, names=(8, 9, 10, 11), inf_at=10):
    rng = np.random.default_rng(3)
    d = os.path.join(root, "scannetpp", "scene")
    for n in names:
        _write_frame(f"{d}/color/{n}.jpg", f"{d}/depth/{n}.png", rng, 24, 16, 24, 16)
        P = np.full((4, 4), np.inf) if n == inf_at else _pose(rng)
        os.makedirs(f"{d}/pose", exist_ok=True)
        np.savetxt(f"{d}/pose/{n}.txt", P)
    os.makedirs(f"{d}/intrinsic", exist_ok=True)
    np.savetxt(f"{d}/intrinsic/intrinsic_depth.txt", np.array([[20.0, 0, 11.5, 0], [0, 21.0, 7.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]]))
    return d


def test_ours_integer_order_and_inf_pose(tmp_path):
    d = _ours(str(tmp_path))
    info = ds.read_ours(d, scannetpp=True)
    ref = _ref_ours(d, 0, -1, 0)
    assert [os.path.basename(f.color_path) for f in info.frames] == ["8.jpg", "9.jpg", "11.jpg"]   # 10: inf pose, skipped
    _check_same(info, ref)
    assert info.depth_scale == 1000.0 and (info.fx, info.fy, info.cx, info.cy) == (20.0, 21.0, 11.5, 7.5)
    assert info.mesh_path == os.path.join(d, "mesh_aligned_cull.ply") and info.type == "Scannetpp"
    assert ds.read_ours(d).mesh_path is None


def test_load_dataset_dispatch_and_rejections(tmp_path):
    scene = _replica(str(tmp_path))
    a = SimpleNamespace(type="Replica", source_path=scene, frame_start=0, frame_num=4, frame_step=0, eval=False, resolution=1,
                        resolution_scales=[1.0])
    assert len(ds.load_dataset(a)) == 4
    with pytest.raises(ValueError, match="eval"):
        ds.load_dataset(SimpleNamespace(**{**vars(a), "eval": True}))
    with pytest.raises(ValueError, match="resize"):
        ds.load_dataset(SimpleNamespace(**{**vars(a), "resolution": 2}))
    assert ds.loadcam_size(1200, 680, 1) == (1200, 680) and ds.loadcam_size(2000, 1000, -1) == (1600, 800)


def test_depth_decode_accepts_i16_and_i32_and_rejects_out_of_range(tmp_path):
    a = np.array([[0, 1, 65535], [300, 40000, 7]], dtype=np.uint16)
    Image.fromarray(a).save(tmp_path / "d.png")
    assert Image.open(tmp_path / "d.png").mode in ("I;16", "I")
    np.testing.assert_array_equal(ds.decode_depth(str(tmp_path / "d.png")), a)
    Image.fromarray(a.astype(np.int32), "I").save(tmp_path / "d32.tif")          # an int32 image: as older Pillow reads PNGs
    assert np.asarray(Image.open(tmp_path / "d32.tif")).dtype == np.int32
    np.testing.assert_array_equal(ds.decode_depth(str(tmp_path / "d32.tif")), a)
    bad = a.astype(np.int32)
    bad[0, 0] = 70000
    Image.fromarray(bad, "I").save(tmp_path / "bad.tif")
    with pytest.raises(ValueError, match="0..65535"):
        ds.decode_depth(str(tmp_path / "bad.tif"))
