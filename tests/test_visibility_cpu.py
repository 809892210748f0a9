"""The visibility rule itself (tests/visibility_reference.py), on cases whose answer is known without it.  No GPU."""
import numpy as np

from rtg_slam_amd import synth
from tests import visibility_reference as vr

F32 = np.float32


def _point_at(K, col, row, z):
    """The point on the ray through the centre of pixel (col, row) at camera depth z."""
    fx, fy, cx, cy = K
    return [(col - cx) / fx * z, (row - cy) / fy * z, z]


def test_occluder_halves():
    H, W = 24, 32
    K = (30.0, 30.0, 15.5, 11.5)
    depth = np.full((H, W), 2.0, F32)
    depth[:, :W // 2] = 1.0
    depth[5, 20] = 0.0                                   # a hole in the right half
    cols, rows = np.meshgrid(np.arange(W), np.arange(H))
    cols, rows = cols.reshape(-1), rows.reshape(-1)
    far = np.array([_point_at(K, c, r, 2.0) for c, r in zip(cols, rows)], dtype=F32)
    near = np.array([_point_at(K, c, r, 1.0) for c, r in zip(cols, rows)], dtype=F32)
    extra = np.array([_point_at(K, 20, 10, -1.0),        # behind the camera
                      _point_at(K, W, 10, 2.0),          # column W: outside
                      _point_at(K, -1, 10, 1.0)], dtype=F32)
    pts = np.concatenate([far, near, extra])
    views = np.zeros(len(pts), np.int32)
    seen = vr.views_add(views, pts, depth, K, np.eye(4), 0.03)
    n = H * W
    left, hole = cols < W // 2, (cols == 20) & (rows == 5)
    assert (views[:n][left] == 0).all()                  # z = 2 behind the 1 m occluder
    assert (views[:n][~left & ~hole] == 1).all()         # z = 2 on the 2 m surface
    assert views[:n][hole].tolist() == [0]               # depth 0 sees nothing
    assert (views[n:2 * n][left] == 1).all()             # z = 1 on the occluder
    assert (views[n:2 * n][~left & ~hole] == 1).all()    # in front of the 2 m surface: free space is not culled
    assert views[2 * n:].tolist() == [0, 0, 0]
    assert seen == int(views.sum())
    vr.views_add(views, pts, depth, K, np.eye(4), 0.03)
    assert views.max() == 2 and (views[:n][left] == 0).all()
    nan = np.array([[np.nan, 0, 1], [0, np.nan, 1], [0, 0, np.nan]], dtype=F32)
    vn = np.zeros(3, np.int32)
    assert vr.views_add(vn, nan, depth, K, np.eye(4), 0.03) == 0 and not vn.any()


def _half_replica():
    c = synth.REPLICA
    return synth.CameraSpec(c.H // 2, c.W // 2, c.fx / 2, c.fy / 2, (c.cx + 0.5) / 2 - 0.5, (c.cy + 0.5) / 2 - 0.5)


def test_box_room_sees_its_part_and_never_the_annex():
    """The 20 frames of the command-line tests (synth.trajectory(20, seed=21), the half-size Replica camera) on the 10 cm
    grid of the flat room and of the cube annex behind its wall.  This restatement gives: 2 638 of the room's 13 166 vertices
    seen at tolerance 0.03 and 2 738 at 0.1; 0 of the annex's 2 646 at either."""
    cam = _half_replica()
    K = (cam.fx, cam.fy, cam.cx, cam.cy)
    v, f, n_room = vr.room_and_annex()
    assert n_room == 13166 and len(v) - n_room == 2646
    tight, loose = np.zeros(len(v), np.int32), np.zeros(len(v), np.int32)
    for p in synth.trajectory(20, seed=21):
        depth = synth.box_room_depth(cam, p).numpy().reshape(cam.H, cam.W)
        vr.views_add(tight, v, depth, K, p.numpy(), 0.03)
        vr.views_add(loose, v, depth, K, p.numpy(), 0.1)
    n_tight, n_loose = int((tight[:n_room] > 0).sum()), int((loose[:n_room] > 0).sum())
    print("room vertices seen:", n_tight, "at 0.03,", n_loose, "at 0.1, of", n_room)
    assert not tight[n_room:].any() and not loose[n_room:].any()
    assert 0 < n_tight < n_room and 0 < n_loose < n_room
    assert (loose >= tight).all()                        # a looser tolerance only ever adds views
    assert tight.max() <= 20 and loose.max() <= 20
    assert (n_tight, n_loose) == (2638, 2738)
    # the culled mesh keeps only faces whose three corners were seen, all of them in the room
    cv, cf = vr.cull_mesh(v, f, loose, 1, False)
    assert 0 < len(cf) < len(f) and cv[:, 0].max() <= 2.5
    assert len(np.unique(cf)) == len(cv)


def test_keep_faces_and_cull_mesh_by_hand():
    v = np.arange(18, dtype=F32).reshape(6, 3)
    f = np.array([[0, 1, 2], [2, 3, 4], [5, 4, 3], [1, 2, 3], [0, 5, 1]], dtype=np.int32)
    views = np.array([2, 1, 2, 0, 2, 1], dtype=np.int32)
    assert vr.keep_faces(f, views, 1, False).tolist() == [1, 0, 0, 0, 1]
    assert vr.keep_faces(f, views, 1, True).tolist() == [1, 1, 1, 1, 1]
    assert vr.keep_faces(f, views, 2, False).tolist() == [0, 0, 0, 0, 0]
    assert vr.keep_faces(f, views, 2, True).tolist() == [1, 1, 1, 1, 1]
    assert vr.keep_faces(f, views, 3, True).tolist() == [0, 0, 0, 0, 0]
    assert vr.keep_faces(f, np.array([0, 0, 0, 0, 2, 0], np.int32), 2, True).tolist() == [0, 1, 1, 0, 0]
    assert vr.keep_faces(np.zeros((0, 3), np.int32), views, 1, False).shape == (0,)
    # all corners, min_views 1: faces 0 and 4 survive in order; vertices 0, 1, 2, 5 in order; 5 -> 3
    cv, cf = vr.cull_mesh(v, f, views, 1, False)
    assert cf.dtype == np.int32 and cf.tolist() == [[0, 1, 2], [0, 3, 1]]
    assert cv.dtype == F32 and np.array_equal(cv, v[[0, 1, 2, 5]])
    # any corner, min_views 2 on a sparser count: faces 1 and 2 survive, vertices 2, 3, 4, 5
    cv, cf = vr.cull_mesh(v, f, np.array([0, 0, 0, 0, 2, 0], np.int32), 2, True)
    assert cf.tolist() == [[0, 1, 2], [3, 2, 1]] and np.array_equal(cv, v[[2, 3, 4, 5]])
    # nothing survives: empty, well-shaped results
    cv, cf = vr.cull_mesh(v, f, views, 3, False)
    assert cv.shape == (0, 3) and cf.shape == (0, 3)
