"""csrc/mesh_render.hip, evaluation.MeshRenderer / mesh_depth_metrics and meshing.cull_unseen against the numpy definition
(tests/mesh_render_reference.py): bit for bit, so every picture is compared with torch.equal."""
import functools

import numpy as np
import pytest
import torch

from rtg_slam_amd import evaluation, meshing, synth
from tests import mesh_render_reference as rr
from tests import visibility_reference as vr

pytestmark = pytest.mark.gpu
F32 = np.float32
# the cameras, the mesh frame and the three poses of tests/test_visibility_gpu.py: TRANSFORM @ POSE0 is the identity exactly
CAMS = {(17, 23): synth.CameraSpec(17, 23, 20.5, 18.25, 10.25, 7.75),
        (48, 64): synth.CameraSpec(48, 64, 60.5, 55.25, 30.25, 25.75)}
TRANSFORM = np.array([[0, -1, 0, 0.5], [1, 0, 0, -0.25], [0, 0, 1, 2.0], [0, 0, 0, 1]], dtype=np.float64)
POSE0 = np.array([[0, 1, 0, 0.25], [-1, 0, 0, 0.5], [0, 0, 1, -2.0], [0, 0, 0, 1]], dtype=np.float64)
SMALL_MAX = (0, 1, 16, 2 ** 30)               # everything queued ... nothing queued
N_VERTS = 300


@functools.lru_cache(maxsize=None)
def _poses():
    assert np.array_equal(TRANSFORM @ POSE0, np.eye(4))
    inv_t = np.linalg.inv(TRANSFORM)
    return [POSE0] + [inv_t @ synth.look_at_pose(seed=s, max_angle_deg=25.0, max_trans=0.4).numpy() for s in (5, 6)]


def _K(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy)


def _reference(cam, v, f, c2w, near=rr.NEAR):
    return rr.render(v, f, _K(cam), cam.H, cam.W, TRANSFORM @ c2w, near)


def _renderer(cam, v, f, **kw):
    return evaluation.MeshRenderer(v, f, cam, transform=TRANSFORM, device="cuda", **kw)


def _same(got, want):
    depth, face = got
    assert depth.dtype == torch.float32 and face.dtype == torch.int32 and depth.shape == face.shape == want[0].shape
    assert torch.equal(face.cpu(), torch.from_numpy(want[1]))
    assert torch.equal(depth.cpu().view(torch.int32), torch.from_numpy(want[0]).view(torch.int32))


@functools.lru_cache(maxsize=None)
def _soup(F, seed=0):
    """300 vertices in a box of the mesh frame that reaches behind the first camera - 60 anywhere, each with four companions
    millimetres to two metres away - and F faces.  Most are an anchor with two of its companions, in either winding: subpixel
    faces, faces of a few pixels, faces larger than the picture, faces across the near plane.  The others are random triples
    (repeated indices included) of the vertices behind the camera or more than 3 m in front of it: dropped, or a backdrop -
    random triples of ALL vertices would put a huge face right before the camera, and the picture would show that face only."""
    rng = np.random.default_rng(seed + F)
    lo, hi = np.array([-3.0, -3.0, -1.0]), np.array([3.0, 3.0, 4.0])
    anchors = lo + rng.random((60, 3)) * (hi - lo)
    reach = 0.005 * 400.0 ** rng.random((60, 1))                              # 5 mm .. 2 m
    v = np.concatenate([anchors] + [anchors + (rng.random((60, 3)) - 0.5) * reach for _ in range(4)])
    assert len(v) == N_VERTS
    back = np.nonzero((v[:, 2] < 0.0) | (v[:, 2] > 3.0))[0]
    f = back[rng.integers(0, len(back), (F, 3))]
    a = rng.integers(0, 60, F)
    j = 1 + rng.integers(0, 4, F)
    k = 1 + (j + rng.integers(0, 3, F)) % 4                                    # another companion than j
    local = rng.random(F) >= 0.15
    f[local] = np.stack([a, a + 60 * j, a + 60 * k], 1)[local]
    return v.astype(F32), f.astype(np.int32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def _soup_reference(shape, F):
    v, f = _soup(F)
    return [_reference(CAMS[shape], v, f, c2w) for c2w in _poses()]


@pytest.mark.parametrize("shape", sorted(CAMS))
@pytest.mark.parametrize("F", [0, 1, 63, 64, 65, 257, 2000])
def test_soups_match_the_definition_whatever_small_max(shape, F):
    cam = CAMS[shape]
    v, f = _soup(F)
    want = _soup_reference(shape, F)
    if F >= 257:
        for w in want:                                                           # neither empty nor one face all over
            assert (w[1] >= 0).any() and (w[1] < 0).any() and len(np.unique(w[1])) > 4
    first = None
    for small_max in SMALL_MAX:
        r = _renderer(cam, v, f, small_max=small_max)
        got = [r.render(c2w) for c2w in _poses()]
        for g, w in zip(got, want):
            _same(g, w)
        if first is None:
            first = got
        for g, g0 in zip(got, first):                                          # and each other
            assert torch.equal(g[0].view(torch.int32), g0[0].view(torch.int32)) and torch.equal(g[1], g0[1])
        assert r.renders == 3 and r.seconds > 0


@pytest.mark.parametrize("shape", sorted(CAMS))
def test_hand_made_faces(shape):
    cam = CAMS[shape]
    v, f = _soup(257)
    n = len(v)
    extra_v = np.array([[-40, -40, 3.75], [80, -40, 3.75], [-40, 80, 3.75],                  # covers the whole picture at pose 0
                        [0, 0, 1], [0.5, 0.5, 1.5], [1, 1, 2],                     # on one line: zero area
                        [np.nan, 0, 1], [0, np.nan, 1], [0, 0, np.nan], [np.inf, 0, 1]], F32)
    extra_f = np.array([[n, n + 1, n + 2], [n + 3, n + 4, n + 5], [n + 3, n + 3, n + 4], [5, 5, 5],
                        [n + 6, n + 3, n + 5], [n + 3, n + 7, n + 5], [n + 3, n + 4, n + 8], [n + 9, n + 3, n + 5]], np.int32)
    v2, f2 = np.concatenate([v, extra_v]), np.concatenate([extra_f[:1], f, extra_f[1:]])
    want = [_reference(cam, v2, f2, c2w) for c2w in _poses()]
    assert (want[0][1] >= 0).all() and (want[0][1] == 0).any()                  # the big triangle: wherever nothing is nearer
    for small_max in SMALL_MAX:
        r = _renderer(cam, v2, f2, small_max=small_max)
        for c2w, w in zip(_poses(), want):
            _same(r.render(c2w), w)
    # the big triangle alone: every pixel, one face, one depth chain
    one = _renderer(cam, extra_v[:3], np.array([[0, 1, 2]], np.int32))
    depth, face = one.render(POSE0)
    _same((depth, face), _reference(cam, extra_v[:3], np.array([[0, 1, 2]]), POSE0))
    assert (face == 0).all() and (depth > 0).all()


@functools.lru_cache(maxsize=None)
def _room():
    gv, gf, n_room = vr.room_and_annex()
    n_room_faces = int((gf < n_room).all(axis=1).sum())
    return gv, gf, n_room, n_room_faces


def test_the_wall_grid_and_the_annex():
    cam = CAMS[(48, 64)]
    gv, gf, n_room, n_room_faces = _room()
    assert (gf[:n_room_faces] < n_room).all() and (gf[n_room_faces:] >= n_room).all()
    wall = _renderer(cam, gv[:n_room], gf[:n_room_faces])
    both = _renderer(cam, gv, gf)
    for c2w in _poses():
        want = _reference(cam, gv, gf, c2w)
        got = both.render(c2w)
        _same(got, want)
        assert (want[1] >= 0).all() and (want[1] < n_room_faces).all()          # closed room: every pixel, never the annex
        got_wall = wall.render(c2w)
        assert torch.equal(got_wall[0], got[0]) and torch.equal(got_wall[1], got[1])
    again = both.render(_poses()[-1])                                            # repeatability
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_no_state_survives_a_render():
    cam = CAMS[(48, 64)]
    va, fa = _soup(2000)
    vb, fb = _soup(65)
    p = _poses()
    wa, wb = _soup_reference((48, 64), 2000), _soup_reference((48, 64), 65)
    a = _renderer(cam, va, fa, small_max=0)                                      # every face through the queue
    _same(a.render(p[0]), wa[0])
    _same(a.render(p[1]), wa[1])
    _same(a.render(p[0]), wa[0])                                                 # the keys of the render before are gone
    b = _renderer(cam, vb, fb, small_max=0)
    _same(b.render(p[0]), wb[0])
    _same(a.render(p[2]), wa[2])
    _same(b.render(p[2]), wb[2])
    # a smaller mesh on the scratch a larger one used: the queue's old entries and count are not read
    small = evaluation.MeshRenderer(vb, fb, cam, transform=TRANSFORM, device="cuda", small_max=0)
    small._scratch = a._scratch
    _same(small.render(p[1]), wb[1])
    _same(a.render(p[1]), wa[1])


def test_mesh_depth_metrics_match_the_definition():
    cam = CAMS[(48, 64)]
    v, f = _soup(2000)
    mesh_depth = _renderer(cam, v, f).render(POSE0)[0]
    rng = np.random.default_rng(3)
    ref = (0.2 + 4.0 * rng.random((cam.H, cam.W))).astype(F32)
    ref[rng.random(ref.shape) < 0.1] = 0.0
    ref[0, :5] = np.nan
    ref[1, 0], ref[1, 1] = F32(0.5), F32(3.5)                                    # at the bounds: out
    for lo, hi in ((0.5, 3.5), (0.0, 100.0), (7.0, 8.0)):
        ratio, l1 = rr.depth_metrics(mesh_depth.cpu().numpy(), ref, lo, hi)
        got = evaluation.mesh_depth_metrics(mesh_depth, torch.from_numpy(ref).cuda(), lo, hi)
        assert set(got) == {"mesh_valid_ratio", "mesh_depth_l1"}
        assert got["mesh_valid_ratio"] == ratio
        assert abs(got["mesh_depth_l1"] - l1) <= 1e-9 * l1
    assert ratio == 0.0 and got["mesh_depth_l1"] == 0.0
    ratio, _ = rr.depth_metrics(mesh_depth.cpu().numpy(), ref, 0.5, 3.5)
    assert 0.05 < ratio < 1.0


def test_cull_unseen_is_the_reference_composition():
    cam = CAMS[(48, 64)]
    gv, gf, n_room, _ = _room()
    colors = np.random.default_rng(5).random((len(gv), 3)).astype(F32)
    poses = _poses()
    wv, wf, views = rr.cull_unseen(gv, gf, _K(cam), cam.H, cam.W, [TRANSFORM @ p for p in poses], 0.1)
    used = np.unique(gf[vr.keep_faces(gf, views, 1, False).astype(bool)])
    v, f, c, stats = meshing.cull_unseen(torch.from_numpy(gv).cuda(), torch.from_numpy(gf).cuda(), torch.from_numpy(colors).cuda(),
                                         cam, poses, 0.1, transform=TRANSFORM)
    assert 0 < len(wf) < len(gf) and used.max() < n_room
    assert torch.equal(f.cpu(), torch.from_numpy(wf)) and torch.equal(v.cpu(), torch.from_numpy(wv))
    assert torch.equal(c.cpu(), torch.from_numpy(colors[used]))
    assert stats["F_removed"] == len(gf) - len(wf) and stats["V_removed"] == len(gv) - len(wv) and stats["poses"] == 3
    assert stats["render_s"] > 0 and abs(stats["tolerance"] - 0.1) < 1e-7
    v2, f2, c2, _ = meshing.cull_unseen(gv, gf, None, cam, poses, 0.1, transform=TRANSFORM)       # arrays, no colours
    assert c2 is None and torch.equal(v2, v) and torch.equal(f2, f)


def test_bad_input_raises_and_launches_nothing():
    cam = CAMS[(17, 23)]
    v, f = _soup(65)
    with pytest.raises(RuntimeError, match="HIP device"):
        evaluation.MeshRenderer(torch.from_numpy(v), f, cam)
    with pytest.raises(RuntimeError, match="HIP device"):
        evaluation.MeshRenderer(v, torch.from_numpy(f), cam)
    with pytest.raises(RuntimeError, match="HIP device"):
        evaluation.MeshRenderer(v, f, cam, device="cpu")
    for bad in ([[0, 1, N_VERTS]], [[-1, 0, 1]]):
        with pytest.raises(ValueError, match="face indices"):
            _renderer(cam, v, np.array(bad, np.int32))
    for near in (0.0, -0.05, float("nan")):
        with pytest.raises(ValueError, match="near"):
            _renderer(cam, v, f, near=near)
    with pytest.raises(ValueError, match="small_max"):
        _renderer(cam, v, f, small_max=-1)
    r = _renderer(cam, v, f)
    with pytest.raises(ValueError, match="4x4"):
        r.render(np.eye(3))
    assert r.renders == 0 and r.seconds == 0.0
    depth = torch.zeros(cam.H, cam.W, device="cuda")
    with pytest.raises(ValueError, match="same"):
        evaluation.mesh_depth_metrics(depth, torch.zeros(cam.H + 1, cam.W, device="cuda"), 0.1, 5.0)
    with pytest.raises(ValueError, match="float32"):
        evaluation.mesh_depth_metrics(depth, depth.double(), 0.1, 5.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        evaluation.mesh_depth_metrics(depth, depth.cpu(), 0.1, 5.0)
