"""The mesher's parts that need no GPU: the mesh PLY writer against the reader, the numpy restatement of marching tetrahedra
(tests/tsdf_reference.py) on a sphere's exact distance field, the command line, and TsdfVolume's refusals."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import io_formats as iof
from tests import tsdf_reference as tr


def test_mesh_ply_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((200, 3)) * 3).astype(np.float32)
    f = rng.integers(0, 200, (333, 3)).astype(np.int32)
    c = rng.random((200, 3)).astype(np.float32)
    path = str(tmp_path / "m.ply")
    iof.save_mesh_ply(path, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c))
    head = open(path, "rb").read(400).split(b"end_header")[0].decode("ascii")
    assert "format binary_little_endian 1.0" in head and "property list uchar int vertex_indices" in head
    assert "property float x" in head and "property uchar red" in head
    v2, f2, c2 = iof.load_mesh_ply(path, with_colors=True)
    assert np.array_equal(v2.astype(np.float32).view(np.uint32), v.view(np.uint32))          # bit-equal
    assert np.array_equal(f2, f.astype(np.int64))
    assert np.abs(c2 - c).max() <= 1.0 / 255.0
    assert len(iof.load_mesh_ply(path)) == 2                                                  # the two-result form is unchanged
    # without colours, and an empty mesh
    iof.save_mesh_ply(path, v, f)
    v3, f3, c3 = iof.load_mesh_ply(path, with_colors=True)
    assert c3 is None and np.array_equal(v3.astype(np.float32), v) and np.array_equal(f3, f)
    iof.save_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32))
    v4, f4 = iof.load_mesh_ply(path)
    assert v4.shape == (0, 3) and f4.shape == (0, 3)
    with pytest.raises(ValueError, match="face indices"):
        iof.save_mesh_ply(path, v, np.array([[0, 1, 200]]))


def test_table_is_generated_and_complete():
    table = tr.make_table()
    assert len(table) == 6 and all(len(row) == 16 for row in table)
    for t, row in enumerate(table):
        for m, tris in enumerate(row):
            n_in = bin(m).count("1")
            assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[n_in]
            for tri in tris:
                assert len(set(tri)) == 3
                for a, b in tri:
                    assert a < b and (a & b) == a                 # an edge runs to a corner that contains its bits
    # the 7 edge classes
    classes = {a ^ b for row in table for tris in row for tri in tris for a, b in tri}
    assert classes == set(range(1, 8))


def test_reference_meshes_a_sphere():
    """Marching tetrahedra of the numpy reference on the exact distance field of a sphere (r = 0.5 m, centre off the grid,
    h = 0.04): closed, genus 0, no degenerate face, vertices within eps = L^2 / (8 (r - L)) of the sphere, L = sqrt(3) h, and
    the signed volume within (1 + eps / r)^3 - 1 of the sphere's.  Measured: V 8826, F 17648, largest deviation 1.19 mm of
    eps 1.39 mm, volume 0.32 % off the sphere's of a bound of 0.84 %."""
    tsdf, weight, rgb = tr.sphere_field()
    v, f, c, keys = tr.extract(tsdf, weight, rgb, tr.SPHERE_LO, tr.SPHERE_H)
    figures = tr.check_sphere_mesh(v, f)
    print(figures)
    assert v.dtype == np.float32 and f.dtype == np.int32 and c.shape == v.shape
    assert (np.diff(keys) > 0).all()
    # the normals point out of the sphere, towards positive tsdf
    a, b, cc = (v[f[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, cc - a)
    assert (np.einsum("ij,ij->i", n, (a + b + cc) / 3 - np.asarray(tr.SPHERE_CENTRE)) > 0).all()
    # colours interpolate the field's: inside its range
    assert c.min() >= rgb.min() - 1e-6 and c.max() <= rgb.max() + 1e-6
    # a cell with an unobserved corner is not meshed: the surface opens there
    weight[20, 20, 33] = 0
    v2, f2, _, _ = tr.extract(tsdf, weight, rgb, tr.SPHERE_LO, tr.SPHERE_H)
    assert 0 < len(f2) < len(f) and (tr.edge_use_counts(f2) == 1).any()


def test_reference_integration_of_a_plane():
    """A fronto-parallel wall at z = 1: the fused tsdf is (1 - z) / trunc at the voxel centres in front of it, clipped to 1,
    untouched behind -trunc; one frame gives weight 1; outside the frustum nothing changes."""
    lo, voxel, trunc = (-0.5, -0.5, 0.0), 0.05, 0.2
    tsdf, weight, rgb = tr.new_volume((20, 20, 30))
    H, W = 60, 80
    depth = np.ones((H, W), np.float32)
    color = np.stack([np.full((H, W), v, np.float32) for v in (0.25, 0.5, 0.75)])
    K = (40.0, 40.0, 39.5, 29.5)
    n = tr.integrate(tsdf, weight, rgb, lo, voxel, trunc, 64, depth, color, K, np.eye(4))
    assert n == int((weight > 0).sum()) and n > 0
    z = np.asarray(tr.axis_centres(lo[2], 30, voxel), dtype=np.float64)
    col = tsdf[:, 10, 10]
    seen = weight[:, 10, 10] > 0
    assert np.array_equal(seen, ((1.0 - z) >= -trunc - 1e-6) & (z > 0.03))   # the nearest centre projects to u = 79.5: pixel 80
    assert np.allclose(col[seen], np.minimum(1.0, (1.0 - z[seen]) / trunc), atol=1e-6)
    assert (col[~seen] == 1).all() and (rgb[:, ~seen, 10, 10] == 0).all()
    assert np.allclose(rgb[:, seen, 10, 10], np.array([0.25, 0.5, 0.75])[:, None])
    assert weight[1, 0, 0] == 0                       # (-0.475, -0.475, 0.075) projects to u = -214: outside the image
    assert set(np.unique(weight)) == {0.0, 1.0}


def test_parser_accepts_mesh_and_metric_mesh():
    from rtg_slam_amd.__main__ import build_parser
    p = build_parser()
    o = p.parse_args(["mesh", "--config", "x.yaml"])
    assert (o.cmd, o.voxel, o.trunc_voxels, o.depth_source, o.every, o.frames, o.min_weight, o.load_frame, o.load_iter,
            o.eval_merge, o.device) == ("mesh", 0.01, 4.0, "render", 1, None, 1.0, -1, [], False, "cuda:0")
    o = p.parse_args(["mesh", "--config", "x.yaml", "--voxel", "0.02", "--trunc-voxels", "3", "--depth-source", "sensor", "--every",
                      "5", "--frames", "100", "--min-weight", "2", "--load-frame", "19", "--load-iter", "30", "40", "--eval-merge",
                      "--io-workers", "2", "--resolution-scale", "2"])
    assert (o.voxel, o.trunc_voxels, o.depth_source, o.every, o.frames, o.min_weight, o.load_frame, o.load_iter, o.eval_merge,
            o.io_workers, o.resolution_scale) == (0.02, 3.0, "sensor", 5, 100, 2.0, 19, [30, 40], True, 2, 2.0)
    with pytest.raises(SystemExit):
        p.parse_args(["mesh", "--config", "x.yaml", "--depth-source", "lidar"])
    assert p.parse_args(["metric", "--config", "x.yaml", "--mesh"]).mesh is True
    assert p.parse_args(["metric", "--config", "x.yaml"]).mesh is False


def test_volume_refuses_an_over_cap_grid_and_cpu_tensors():
    from rtg_slam_amd import meshing
    with pytest.raises(ValueError, match=r"1000 x 1000 x 1000 grid.*18\.63 GiB.*cap of 16\.00 GiB"):
        meshing.TsdfVolume((0, 0, 0), (10, 10, 10), 0.01, device="cuda:0")
    with pytest.raises(ValueError, match=r"GiB"):
        meshing.TsdfVolume((0, 0, 0), (1, 1, 1), 0.01, device="cuda:0", max_bytes=1 << 20)
    with pytest.raises(RuntimeError, match="HIP device"):
        meshing.TsdfVolume((0, 0, 0), (1, 1, 1), 0.1, device="cpu")
    t, w, c = (torch.from_numpy(a) for a in tr.new_volume((4, 5, 6)))
    with pytest.raises(RuntimeError, match="HIP device"):
        meshing.TsdfVolume.from_tensors(t, w, c, (0, 0, 0), 0.1)
    assert meshing._intrinsics(np.array([[5.0, 0, 2], [0, 6, 3], [0, 0, 1]])) == (5.0, 6.0, 2.0, 3.0)
