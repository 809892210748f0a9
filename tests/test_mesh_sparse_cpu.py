"""The sparse brick TSDF volume's definition (tests/tsdf_sparse_reference.py) against the dense one (tests/tsdf_reference.py),
without a GPU: brick counts, the one-frame theorems, which voxels differ after several frames, grids that are no multiple of
the brick, the command line and SparseTsdfVolume's refusals."""
import numpy as np
import pytest
import torch

from tests import tsdf_reference as tr
from tests import tsdf_sparse_reference as ts

F = np.float32


def _both(cam, frames, lo, dims, voxel, trunc):
    """Sparse and dense references fused side by side; yields (sparse volume, dense planes) after every frame."""
    vol = ts.SparseVolume(lo, dims, voxel, trunc)
    dense = tr.new_volume(dims)
    K = (cam.fx, cam.fy, cam.cx, cam.cy)
    for depth, color, c2w in frames:
        d = np.asarray(depth, dtype=F).reshape(cam.H, cam.W)
        c = np.asarray(color, dtype=F)
        vol.integrate(d, c, K, c2w)
        tr.integrate(*dense, [float(F(x)) for x in lo], F(voxel), F(trunc), F(64), d, c, K, c2w)
        yield vol, dense


def _differing(vol, dense):
    """[nz, ny, nx] bool: allocated voxels whose tsdf, weight or rgb differ from the dense volume's (by bits)."""
    t, w, c = vol.to_dense()
    diff = (t.view(np.uint32) != dense[0].view(np.uint32)) | (w.view(np.uint32) != dense[1].view(np.uint32))
    diff |= (c.view(np.uint32) != dense[2].view(np.uint32)).any(axis=0)
    return diff & vol.allocated_voxels()


def _assert_mesh_equals_dense(vol, dense, lo, voxel):
    got = vol.extract()
    want = tr.extract(dense[0], dense[1], dense[2], [F(x) for x in lo], F(voxel))
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b)
    return got


def _numpy_frames(frames):
    return [(d.numpy(), c.numpy(), p) for d, c, p in frames]


def test_three_frames_brick_counts_and_theorems():
    """dims (96, 64, 112) at 5 cm, 1 344 bricks.  One frame: 210 bricks, no allocated voxel differs from the dense volume, the
    mesh is the dense reference's bit for bit (V 29 304, F 57 908).  Three frames: 309 bricks; 1 155 of 158 208 allocated
    voxels differ, exactly the ones the dense rule updated before their brick was allocated; the mesh is identical on these
    inputs (V 41 582, F 81 098), which is an observation, not a property."""
    cam, frames = ts.three_frames()
    dims = (96, 64, 112)
    assert np.prod(ts.brick_dims(dims)) == 1344
    steps = _both(cam, _numpy_frames(frames), ts.THREE_LO, dims, ts.THREE_VOXEL, 4 * ts.THREE_VOXEL)
    vol, dense = next(steps)
    assert vol.n_bricks == 210 and int(vol.allocated_voxels().sum()) == 107520
    assert int(_differing(vol, dense).sum()) == 0 and not vol.lost[vol.allocated_voxels()].any()
    v, f, _, _ = _assert_mesh_equals_dense(vol, dense, ts.THREE_LO, ts.THREE_VOXEL)
    assert (len(v), len(f)) == (29304, 57908)
    order = (vol.brick_coords[:, 2].astype(np.int64) * 8 + vol.brick_coords[:, 1]) * 12 + vol.brick_coords[:, 0]
    assert (np.diff(order) > 0).all()                                   # one frame: slots in ascending brick linear index
    next(steps)
    vol, dense = next(steps)
    assert vol.n_bricks == 309 and int(vol.allocated_voxels().sum()) == 158208
    diff = _differing(vol, dense)
    print("differing voxels in allocated bricks:", int(diff.sum()))
    assert np.array_equal(diff, vol.lost & vol.allocated_voxels())
    assert int(diff.sum()) == 1155
    assert len(np.unique(vol.brick_coords, axis=0)) == 309
    v, f, _, _ = _assert_mesh_equals_dense(vol, dense, ts.THREE_LO, ts.THREE_VOXEL)
    assert (len(v), len(f)) == (41582, 81098)


def test_box_room_twenty_frames():
    """tr.box_room_case(20): 260 x 160 x 110 at 2 cm, 9 240 bricks; 1 903 allocated after one frame, 2 243 after 20 (24 %, where
    the dense form has updated 55 % of the voxels).  The 20-frame mesh: V 229 226, F 456 214, wall statistics equal to the
    dense reference's (mean 0.01126, p99 0.03607, covered 0.184)."""
    cam, frames, lo, hi, voxel = tr.box_room_case(20)
    dims = (260, 160, 110)
    assert np.prod(ts.brick_dims(dims)) == 9240
    lo32 = [F(x) for x in lo]
    counts = []
    for vol, dense in _both(cam, _numpy_frames(frames), lo32, dims, F(voxel), F(4 * voxel)):
        counts.append(vol.n_bricks)
    print("bricks per frame:", counts, "dense share updated:", float((dense[1] > 0).mean()))
    assert counts[0] == 1903 and counts[-1] == 2243
    assert 0.23 < counts[-1] / 9240 < 0.25 and 0.54 < (dense[1] > 0).mean() < 0.56
    diff = _differing(vol, dense)
    assert np.array_equal(diff, vol.lost & vol.allocated_voxels())
    v, f, _, _ = vol.extract()
    rv, rf, _, _ = tr.extract(dense[0], dense[1], dense[2], lo32, F(voxel))
    assert (len(v), len(f)) == (229226, 456214) and (len(rv), len(rf)) == (len(v), len(f))
    got, want = tr.wall_stats(v), tr.wall_stats(rv)
    print("sparse:", got, "dense:", want)
    for k in ("mean", "p99", "covered"):
        assert got[k] == want[k], (k, got[k], want[k])


@pytest.mark.parametrize("dims", [(61, 45, 83), (93, 59, 109)])
def test_dims_that_are_no_multiple_of_the_brick(dims):
    """dims (61, 45, 83), which the first frame misses altogether and the other two graze (14 and 6 bricks), and (93, 59, 109),
    which cuts the last brick of every axis where the walls are: the one-frame theorems hold for every first frame, and the
    cut bricks' voxels outside the grid do not exist - the planes have the grid's shape, the allocation mask is cut to it."""
    cam, frames = ts.three_frames()
    frames = _numpy_frames(frames)
    nb = ts.brick_dims(dims)
    shape = dims[::-1]
    bricks = []
    for k in range(3):
        vol, dense = next(_both(cam, frames[k:k + 1], ts.THREE_LO, dims, ts.THREE_VOXEL, 4 * ts.THREE_VOXEL))
        bricks.append(vol.n_bricks)
        assert vol.tsdf.shape == shape and vol.allocated_voxels().shape == shape
        assert int(_differing(vol, dense).sum()) == 0
        v, f, _, keys = _assert_mesh_equals_dense(vol, dense, ts.THREE_LO, ts.THREE_VOXEL)
        b = vol.brick_coords
        assert (b >= 0).all() and all((b[:, a] < nb[a]).all() for a in range(3))
        if vol.n_bricks:
            assert len(f) > 0 and keys.max() // 7 < np.prod(dims)
            assert (b[:, 0] == nb[0] - 1).any() and (b[:, 2] == nb[2] - 1).any()        # cut bricks are in use
    print("bricks after each frame alone:", bricks)
    assert bricks == [0, 14, 6] if dims == (61, 45, 83) else min(bricks) > 100
    for vol, dense in _both(cam, frames, ts.THREE_LO, dims, ts.THREE_VOXEL, 4 * ts.THREE_VOXEL):
        pass
    assert np.array_equal(_differing(vol, dense), vol.lost & vol.allocated_voxels())
    t, w, c = vol.to_dense()
    un = ~vol.allocated_voxels()
    assert (t[un] == 1).all() and (w[un] == 0).all() and (c[:, un] == 0).all()


def test_window_of_the_grid_equals_the_whole():
    """The window form (true indices) on a grid small enough to hold: the same bricks, planes and mesh."""
    cam, frames = ts.three_frames()
    dims = (96, 64, 112)
    frames = _numpy_frames(frames)[:1]
    whole, _ = ts.fuse_sparse(cam, frames, ts.THREE_LO, dims, ts.THREE_VOXEL, 4 * ts.THREE_VOXEL)
    b = whole.brick_coords
    window = tuple((max(0, int(b[:, a].min()) * 8 - 8), min((int(b[:, a].max()) + 1) * 8 + 8, dims[a])) for a in range(3))
    assert all(lo >= 0 for lo, _ in window) and any(lo > 0 for lo, _ in window)
    part, _ = ts.fuse_sparse(cam, frames, ts.THREE_LO, dims, ts.THREE_VOXEL, 4 * ts.THREE_VOXEL, window=window)
    assert np.array_equal(part.brick_coords, whole.brick_coords)
    (x0, x1), (y0, y1), (z0, z1) = window
    for a, b in zip(part.to_dense(), whole.to_dense()):
        assert np.array_equal(a, b[..., z0:z1, y0:y1, x0:x1])
    for a, b in zip(part.extract(), whole.extract()):
        assert np.array_equal(a, b)


def test_parser_accepts_volume():
    from rtg_slam_amd.__main__ import build_parser
    p = build_parser()
    assert p.parse_args(["mesh", "--config", "x.yaml"]).volume == "dense"
    assert p.parse_args(["mesh", "--config", "x.yaml", "--volume", "sparse"]).volume == "sparse"
    assert p.parse_args(["mesh", "--config", "x.yaml", "--volume", "dense"]).volume == "dense"
    with pytest.raises(SystemExit):
        p.parse_args(["mesh", "--config", "x.yaml", "--volume", "foo"])


def test_sparse_volume_refuses_cpu():
    from rtg_slam_amd import meshing
    with pytest.raises(RuntimeError, match="HIP device"):
        meshing.SparseTsdfVolume((0, 0, 0), (1, 1, 1), 0.1, device="cpu")
    with pytest.raises(ValueError, match="brick table"):
        meshing.SparseTsdfVolume((0, 0, 0), (10, 10, 10), 0.01, device="cuda:0", max_bytes=1 << 20)
    with pytest.raises(ValueError, match="mesh_from_map"):
        meshing.mesh_from_map(None, None, [np.eye(4)], None, volume="hashed", bounds=((0, 0, 0), (1, 1, 1)))
    vol = meshing.SparseTsdfVolume((0, 0, 0), (1, 1, 1), 0.1, device="cuda:0")      # nothing is allocated before the first frame
    with pytest.raises(RuntimeError, match="HIP device"):
        vol.integrate(torch.zeros(4, 4), torch.zeros(3, 4, 4), (1.0, 1.0, 1.0, 1.0), np.eye(4))
