"""Evaluation without a GPU: the float64 restatement (tests/eval_reference.py) against the reference's own loss functions and
its stated properties, the mesh / metrics-table formats of rtg_slam_amd.io_formats, and the host-side refusals of
rtg_slam_amd.evaluation."""
import csv
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from rtg_slam_amd import io_formats as iof
from tests import eval_reference as er

REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
def test_restatement_psnr_and_l1_equal_the_references_loss_utils():
    spec = importlib.util.spec_from_file_location("ref_loss_utils", os.path.join(REF, "utils", "loss_utils.py"))
    lu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lu)
    g = torch.Generator().manual_seed(3)
    for H, W in ((17, 23), (64, 48)):
        a = torch.rand(3, H, W, generator=g, dtype=torch.float64)
        b = (a + 0.1 * torch.randn(3, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
        ref_psnr = lu.psnr(a, b)                                # [3, 1]: per channel; eval.py takes .mean()
        assert np.allclose(er.psnr_per_channel(a.numpy(), b.numpy()), ref_psnr.reshape(-1).numpy(), rtol=0, atol=1e-10)
        assert abs(er.psnr(a.numpy(), b.numpy()) - float(ref_psnr.mean())) < 1e-10
        assert abs(er.l1_loss(a.numpy(), b.numpy()) - float(lu.l1_loss(a, b))) < 1e-14
        # the ad-hoc whole-image PSNR is never above the reference's mean of per-channel PSNRs (Jensen)
        whole = 10 * math.log10(1.0 / float(((a - b) ** 2).mean()))
        assert whole <= er.psnr(a.numpy(), b.numpy()) + 1e-12


def test_restatement_ms_ssim_properties():
    rng = np.random.default_rng(0)
    x = rng.random((3, 200, 230))
    assert abs(er.ms_ssim(x, x) - 1.0) < 1e-12
    y = np.clip(x + 0.05 * rng.standard_normal(x.shape), 0, 1)
    v = er.ms_ssim(x, y)
    assert 0.0 < v < 1.0
    assert er.level_sizes(680, 1200) == [(680, 1200), (340, 600), (170, 300), (85, 150), (43, 75)]
    assert er.level_sizes(341, 517) == [(341, 517), (171, 259), (86, 130), (43, 65), (22, 33)]
    # pooling: odd axes padded by one zero in front, divisor 4
    p = er.avg_pool(np.arange(15, dtype=np.float64).reshape(1, 3, 5))
    assert p.shape == (1, 2, 3)
    assert p[0, 0, 0] == 0.0 / 4 and p[0, 0, 1] == (1 + 2) / 4 and p[0, 1, 2] == (8 + 9 + 13 + 14) / 4
    with pytest.raises(ValueError):
        er.ms_ssim(np.zeros((3, 160, 300)), np.zeros((3, 160, 300)))
    er.ms_ssim(np.zeros((3, 161, 300)), np.zeros((3, 161, 300)))


def _cube(quads: bool):
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)
    q = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]])
    if quads:
        return v, q
    return v, np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])


def _write_mesh(path, v, f, binary):
    head = ["ply", "format binary_little_endian 1.0" if binary else "format ascii 1.0", "comment cube",
            f"element vertex {len(v)}", "property float x", "property float y", "property float z", "property uchar red",
            f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        if binary:
            vt = np.zeros(len(v), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1")])
            vt["x"], vt["y"], vt["z"], vt["r"] = v[:, 0], v[:, 1], v[:, 2], 7
            fh.write(vt.tobytes())
            for face in f:
                fh.write(np.uint8(len(face)).tobytes() + np.asarray(face, "<i4").tobytes())
        else:
            for p in v:
                fh.write(f"{p[0]} {p[1]} {p[2]} 7\n".encode())
            for face in f:
                fh.write((f"{len(face)} " + " ".join(str(int(i)) for i in face) + "\n").encode())


def _tri_set(f):
    return sorted(tuple(sorted(t)) for t in np.asarray(f).tolist())


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("quads", [False, True])
def test_load_mesh_ply_round_trips_a_cube(tmp_path, binary, quads):
    v, f = _cube(quads)
    path = str(tmp_path / "cube.ply")
    _write_mesh(path, v, f, binary)
    vv, ff = iof.load_mesh_ply(path)
    assert vv.dtype == np.float64 and np.array_equal(vv, v)
    assert ff.shape == (12, 3)
    assert _tri_set(ff) == _tri_set(_cube(False)[1])
    # mixed triangles and quads in one face list (row-by-row path)
    mixed = [list(q) for q in _cube(True)[1][:3]] + [list(t) for t in _cube(False)[1][[3, 9, 4, 10, 5, 11]]]
    _write_mesh(path, v, mixed, binary)
    _, fm = iof.load_mesh_ply(path)
    assert _tri_set(fm) == _tri_set(_cube(False)[1])


def test_sample_mesh_surface_lies_on_faces_and_follows_area():
    # two triangles of area 1 and 3 (z = 0 and x = 5 planes)
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [5, 0, 0], [5, 3, 0], [5, 0, 2]], dtype=np.float64)
    f = np.array([[0, 1, 2], [3, 4, 5]])
    n = 40000
    pts, face = iof.sample_mesh_surface(v, f, n, seed=1)
    assert pts.shape == (n, 3) and face.shape == (n,)
    for k in range(2):
        a, b, c = v[f[k]]
        p = pts[face == k]
        # barycentric coordinates of each point in its face: in the triangle, on its plane
        M = np.stack([b - a, c - a], axis=1)
        uv, res, *_ = np.linalg.lstsq(M, (p - a).T, rcond=None)
        assert np.abs(M @ uv - (p - a).T).max() < 1e-12
        assert uv.min() >= -1e-12 and (uv.sum(0)).max() <= 1 + 1e-12
    # counts follow area (1 : 3): binomial sd = sqrt(n p (1 - p)) ~ 87; allow 5 sd
    assert abs(int((face == 1).sum()) - 0.75 * n) < 5 * math.sqrt(n * 0.75 * 0.25)
    assert np.array_equal(iof.sample_mesh_surface(v, f, 100, seed=4)[0], iof.sample_mesh_surface(v, f, 100, seed=4)[0])


def test_save_metrics_csv_writes_rows_and_the_mean_row(tmp_path):
    rows = [dict(valid_pixel_ratio=0.5, depth_loss=0.01, normal_loss=0, psnr=30.0, ssim=0.9, lpips=None, frame=0, iter=0),
            dict(valid_pixel_ratio=0.7, depth_loss=float("nan"), normal_loss=0, psnr=32.0, ssim=0.95, lpips=None, frame=1,
                 iter=0, accuracy=1.5)]
    path = str(tmp_path / "out" / "statis.csv")
    iof.save_metrics_csv(path, rows)
    with open(path) as fh:
        table = list(csv.reader(fh))
    cols = ["valid_pixel_ratio", "depth_loss", "normal_loss", "psnr", "ssim", "lpips", "frame", "iter", "accuracy"]
    assert table[0] == [""] + cols
    assert [r[0] for r in table[1:]] == ["0", "1", "2"]
    mean = dict(zip(table[0], table[3]))
    assert mean["frame"] == "mean"
    assert float(mean["psnr"]) == 31.0 and abs(float(mean["valid_pixel_ratio"]) - 0.6) < 1e-15
    assert float(mean["depth_loss"]) == 0.01                   # NaN skipped, as pandas' mean
    assert float(mean["accuracy"]) == 1.5 and mean["lpips"] == ""
    assert dict(zip(table[0], table[2]))["depth_loss"] == "" and dict(zip(table[0], table[1]))["accuracy"] == ""


def test_eval_picture_refuses_small_images_and_cpu_tensors():
    from rtg_slam_amd import evaluation as ev
    H, W = 160, 300
    out = {"render": torch.zeros(3, H, W), "depth": torch.zeros(1, H, W), "depth_index_map": torch.zeros(1, H, W, dtype=torch.int32)}
    with pytest.raises(ValueError, match="160"):
        ev.eval_picture(out, torch.zeros(3, H, W), torch.zeros(H, W), 0.1, 5.0)
    H = 161
    out = {"render": torch.zeros(3, H, W), "depth": torch.zeros(1, H, W), "depth_index_map": torch.zeros(1, H, W, dtype=torch.int32)}
    with pytest.raises(RuntimeError, match="HIP device"):
        ev.eval_picture(out, torch.zeros(3, H, W), torch.zeros(H, W), 0.1, 5.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ev.eval_pcd(torch.zeros(10, 3), torch.zeros(10, 3))
