"""tests/mesh_render_reference.py - the definition csrc/mesh_render.hip is held to - against facts: the analytic box room,
hand-made triangles whose float chains are exact, a welded plane without cracks, a depth L1 worked by hand and the cull of
the annex no pose can see.  No GPU."""
import numpy as np
import pytest

from rtg_slam_amd import synth
from tests import mesh_render_reference as rr
from tests import visibility_reference as vr

F32 = np.float32
CAM = synth.CameraSpec(48, 64, 60.5, 55.25, 30.25, 25.75)               # the (48, 64) camera of tests/test_visibility_gpu.py
# the hand-made cases: every entry a power of two or a small integer, so u = 16 x / z + 8 is exact at z = 1 and 2
HAND = synth.CameraSpec(12, 16, 16.0, 16.0, 8.0, 6.0)
EYE = np.eye(4)


def _K(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy)


def _at(u, v, z):
    """The point of the identity camera HAND that projects to (u, v) at depth z."""
    return [(u - 8.0) * z / 16.0, (v - 6.0) * z / 16.0, z]


def _hand(vertices, faces, near=rr.NEAR):
    return rr.render(np.asarray(vertices, F32), np.asarray(faces, np.int32).reshape(-1, 3), _K(HAND), HAND.H, HAND.W, EYE, near)


def _grid():
    return np.meshgrid(np.arange(HAND.H), np.arange(HAND.W), indexing="ij")                    # rows (v), columns (u)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_wall_grid_is_the_box_room(seed):
    pose = synth.look_at_pose(seed=seed, max_angle_deg=40.0, max_trans=0.8)
    gv, gf = vr.box_grid(vr.ROOM_HALF)
    depth, face = rr.render(gv, gf, _K(CAM), CAM.H, CAM.W, pose.numpy())
    want = synth.box_room_depth(CAM, pose, bump=0.0)[..., 0].numpy()
    assert depth.dtype == F32 and face.dtype == np.int32 and depth.shape == (CAM.H, CAM.W)
    assert (depth > 0).all() and (face >= 0).all() and face.max() < len(gf)
    rel = np.abs(depth.astype(np.float64) - want) / want
    print("largest relative difference", rel.max())
    assert rel.max() < 2e-6


@pytest.mark.parametrize("winding", [(0, 1, 2), (0, 2, 1)])
def test_corners_and_edges_on_pixel_centres_are_covered(winding):
    depth, face = _hand([_at(2, 1, 2.0), _at(10, 1, 2.0), _at(2, 9, 2.0)], [winding])
    r, c = _grid()
    inside = (c >= 2) & (r >= 1) & ((c - 2) + (r - 1) <= 8)                  # the closed triangle: edges and corners included
    assert inside[1, 2] and inside[1, 10] and inside[9, 2] and inside[5, 6]
    assert np.array_equal(face, np.where(inside, 0, -1))
    assert np.array_equal(depth, np.where(inside, F32(2), F32(0)))           # z exact: every w an integer, iz = 0.5


def test_coplanar_copies_the_lower_index_wins():
    tri = [_at(2, 1, 2.0), _at(10, 1, 2.0), _at(2, 9, 2.0)]
    one, _ = _hand(tri, [(0, 1, 2)])
    depth, face = _hand(tri + tri, [(3, 4, 5), (0, 1, 2), (5, 4, 3)])
    assert np.array_equal(depth, one) and set(np.unique(face)) == {-1, 0}
    assert np.array_equal(face >= 0, one > 0)


def test_the_nearer_triangle_hides_the_farther():
    far = [_at(1, 1, 2.0), _at(14, 1, 2.0), _at(1, 11, 2.0)]
    near = [_at(3, 2, 1.0), _at(7, 2, 1.0), _at(3, 6, 1.0)]
    for faces, (i_far, i_near) in (([(0, 1, 2), (3, 4, 5)], (0, 1)), ([(3, 4, 5), (0, 1, 2)], (1, 0))):
        depth, face = _hand(far + near, faces)
        r, c = _grid()
        in_near = (c >= 3) & (r >= 2) & ((c - 3) + (r - 2) <= 4)
        in_far = (c >= 1) & (r >= 1) & (10 * (c - 1) + 13 * (r - 1) <= 130)
        assert np.array_equal(face, np.where(in_near, i_near, np.where(in_far, i_far, -1)))
        assert np.array_equal(depth, np.where(in_near, F32(1), np.where(in_far, F32(2), F32(0))))


def test_a_corner_at_the_near_plane_drops_the_face():
    near = F32(rr.NEAR)
    rest = [_at(2, 1, 2.0), _at(10, 9, 2.0)]
    depth, face = _hand([[0, 0, near]] + rest, [(0, 1, 2)])
    assert not depth.any() and (face == -1).all()
    depth, face = _hand([[0, 0, np.nextafter(near, F32(1))]] + rest, [(0, 1, 2)])
    assert (face == 0).any() and (depth[face == 0] > 0).all()
    depth, face = _hand([[0, 0, 0.25]] + rest, [(0, 1, 2)], near=0.25)          # the same at another near
    assert (face == -1).all()


def test_degenerate_and_nan_faces_draw_nothing_and_harm_nothing():
    tri = [_at(2, 1, 2.0), _at(10, 1, 2.0), _at(2, 9, 2.0)]
    one_d, one_f = _hand(tri, [(0, 1, 2)])
    depth, face = _hand(tri, [(0, 0, 1)])                                    # a repeated corner
    assert (face == -1).all() and not depth.any()
    depth, face = _hand(tri + [_at(2, 1, 1.0)], [(3, 0, 1)])                  # two corners that project to one point
    assert (face == -1).all()
    depth, face = _hand(tri + [_at(6, 1, 2.0)], [(0, 3, 1)])                  # zero area: three corners on one line
    assert (face == -1).all()
    for k in range(3):
        bad = _at(6, 5, 1.0)
        bad[k] = np.nan
        depth, face = _hand(tri + [bad], [(3, 1, 2), (0, 1, 2), (0, 3, 2)])
        assert np.array_equal(depth, one_d) and np.array_equal(face, np.where(one_f == 0, 1, -1))
    depth, face = _hand(tri + [[np.inf, 0, 1.0]], [(3, 1, 2)])
    assert (face == -1).all()


def test_a_face_off_the_image_and_a_box_wider_than_it():
    depth, face = _hand([_at(-9, 1, 2.0), _at(-2, 1, 2.0), _at(-9, 9, 2.0)], [(0, 1, 2)])
    assert (face == -1).all() and not depth.any()
    depth, face = _hand([_at(20, 20, 2.0), _at(30, 20, 2.0), _at(20, 30, 2.0)], [(0, 1, 2)])
    assert (face == -1).all()
    W = HAND.W
    depth, face = _hand([_at(-3, 2, 2.0), _at(W + 3, 2, 2.0), _at(-3, 13, 2.0)], [(0, 1, 2)])
    r, c = _grid()
    inside = (r >= 2) & ((c + 3) + 2 * (r - 2) <= W + 6)                       # the hypotenuse from (W + 3, 2) to (-3, 13)
    assert inside[2, 0] and inside[2, W - 1] and inside[HAND.H - 1, 0] and not inside[HAND.H - 1, W - 1]
    assert np.array_equal(face, np.where(inside, 0, -1)) and np.array_equal(depth, np.where(inside, F32(2), F32(0)))


def jittered_plane(n=41, seed=11):
    """A welded n x n vertex grid across the frustum of CAM at z ~ 2, every vertex jittered in all three axes."""
    rng = np.random.default_rng(seed)
    step = 3.0 / (n - 1)
    g = -1.5 + step * np.arange(n)
    p = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.full((n, n), 2.0)], -1).reshape(-1, 3)
    p[:, :2] += (rng.random((n * n, 2)) - 0.5) * 0.6 * step
    p[:, 2] += (rng.random(n * n) - 0.5) * 0.1
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    q = (i * n + j).reshape(-1)
    faces = np.concatenate([np.stack([q, q + n, q + n + 1], 1), np.stack([q, q + n + 1, q + 1], 1)])
    return p.astype(F32), faces.astype(np.int32)


def test_a_welded_plane_has_no_cracks():
    v, f = jittered_plane()
    for pose in (EYE, synth.look_at_pose(seed=4, max_angle_deg=8.0, max_trans=0.1).numpy()):
        depth, face = rr.render(v, f, _K(CAM), CAM.H, CAM.W, pose)
        assert (face >= 0).all() and (depth > 1.8).all() and (depth < 2.3).all()


def test_depth_metrics_by_hand():
    mesh = np.array([[1.0, 2.0, 0.0, 3.0], [1.5, 0.0, 2.5, 4.0], [2.0, 2.0, 2.0, 2.0]], F32)
    ref = np.array([[1.25, 0.5, 1.0, 5.0], [1.0, 1.0, 2.0, 4.5], [0.0, np.nan, 2.0, 3.0]], F32)
    # min 0.5, max 5.0: (0,1) sits at min and (0,3) at max - both out; (0,2) and (1,1) have no mesh depth; (2,0) and (2,1)
    # have no reference.  Valid: (0,0) 0.25, (1,0) 0.5, (1,2) 0.5, (1,3) 0.5, (2,2) 0, (2,3) 1
    ratio, l1 = rr.depth_metrics(mesh, ref, 0.5, 5.0)
    assert ratio == 6 / 12 and l1 == 2.75 / 6
    assert rr.depth_metrics(mesh, ref, 5.0, 6.0) == (0.0, 0.0)
    assert rr.depth_metrics(np.zeros((3, 4), F32), ref, 0.5, 5.0) == (0.0, 0.0)


def test_cull_unseen_removes_the_annex():
    gv, gf, n_room = vr.room_and_annex()
    poses = [p.numpy() for p in synth.trajectory(20, seed=21)]
    ov, of, views = rr.cull_unseen(gv, gf, _K(CAM), CAM.H, CAM.W, poses, 0.1)
    keep = vr.keep_faces(gf, views, 1, False).astype(bool)
    assert 0 < keep.sum() < len(gf) and len(of) == keep.sum()
    assert not keep[(gf >= n_room).any(axis=1)].any()                        # the wall is more than a metre in front of it
    assert not (ov[:, 0] > 2.6).any()
    assert (views[gf[keep]] >= 1).all()
    used = np.unique(gf[keep])
    assert np.array_equal(ov, gv[used]) and np.array_equal(ov[of], gv[gf[keep]])


def test_the_abi_refuses_before_it_launches():
    """rtgs_mesh_render returns -1, and rtgs_mesh_render_scratch_bytes 0, for the sizes and settings it must not run with; every
    pointer is null, so nothing can have been launched."""
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from rtg_slam_amd import _lib
    lib = _lib.load()
    m = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    one = C.c_void_p(8)                                   # a non-null pointer that is never followed

    def call(V=3, F=1, H=4, W=4, near=0.05, small_max=16, w2c=m, vertices=one, faces=one, scratch=one, depth=one, face=one):
        return lib.rtgs_mesh_render(vertices, V, faces, F, H, W, 16.0, 16.0, 2.0, 2.0, w2c, near, small_max, scratch, depth, face, None)

    assert call(F=2 ** 31) == -1 and call(F=-1) == -1 and call(V=-1) == -1
    assert call(H=65536, W=32768) == -1 and call(H=0) == -1 and call(W=-4) == -1
    assert call(near=0.0) == -1 and call(near=-1.0) == -1 and call(near=float("nan")) == -1
    assert call(small_max=-1) == -1
    assert call(w2c=None) == -1 and call(scratch=None) == -1 and call(depth=None) == -1 and call(face=None) == -1
    assert call(vertices=None) == -1 and call(faces=None) == -1 and call(V=0) == -1
    assert lib.rtgs_mesh_render_scratch_bytes(3, 2 ** 31, 4, 4) == 0 and lib.rtgs_mesh_render_scratch_bytes(3, 1, 65536, 32768) == 0
    assert lib.rtgs_mesh_render_scratch_bytes(3, 5, 4, 6) >= 8 * 24 + 4 * 5 + 4
