"""csrc/visibility.hip and evaluation.VisibilityCull against the numpy definition (tests/visibility_reference.py): bit for
bit, so every comparison is torch.equal."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import evaluation, mesh_ops, synth
from tests import visibility_reference as vr

pytestmark = pytest.mark.gpu
F32 = np.float32
TOL = 0.03
N_EDGE = 9
# fx != fy, an off-centre principal point; every entry has a short mantissa, so the hand-placed chains below are exact
CAMS = {(17, 23): synth.CameraSpec(17, 23, 20.5, 18.25, 10.25, 7.75),
        (48, 64): synth.CameraSpec(48, 64, 60.5, 55.25, 30.25, 25.75)}
# the mesh's frame is the first camera's, turned a quarter about z and shifted by dyadic amounts: TRANSFORM @ POSE0 is the
# identity exactly, so the first frame's matrix is the identity and the hand-placed points meet the edges they are built for
TRANSFORM = np.array([[0, -1, 0, 0.5], [1, 0, 0, -0.25], [0, 0, 1, 2.0], [0, 0, 0, 1]], dtype=np.float64)
POSE0 = np.array([[0, 1, 0, 0.25], [-1, 0, 0, 0.5], [0, 0, 1, -2.0], [0, 0, 0, 1]], dtype=np.float64)


def _poses():
    assert np.array_equal(TRANSFORM @ POSE0, np.eye(4))
    inv_t = np.linalg.inv(TRANSFORM)
    return [POSE0] + [inv_t @ synth.look_at_pose(seed=s, max_angle_deg=25.0, max_trans=0.4).numpy() for s in (5, 6)]


def _edge_points(cam):
    """At the identity matrix, in float32 -> (points [N_EDGE,3], the pixels to set as (row, col, depth), what frame 0 sees)."""
    fx, cx, W = F32(cam.fx), F32(cam.cx), cam.W
    s = F32(8.0 if W == 23 else 32.0)
    t = F32(TOL)
    row = int(np.floor(F32(cam.cy) + F32(0.5)))
    col = int(np.floor(cx + F32(0.5)))
    half = int(fx * F32(0.5) + cx + F32(0.5))                         # u + 0.5 is this integer exactly
    assert F32(half) == fx * F32(0.5) + cx + F32(0.5) and 0 < half < W
    zl = fx / s
    xl, xr = -(cx + F32(0.5)) / s, (F32(W) - F32(0.5) - cx) / s
    assert fx * xl / zl + cx == F32(-0.5) and fx * xr / zl + cx == F32(W) - F32(0.5)
    z_eq, z_above = F32(2) * t, np.nextafter(F32(2) * t, F32(1))
    assert z_eq - t == t and z_above - t > t
    pts = np.array([[0.5, 0, 1],                  # u + 0.5 an integer: floor takes it, pixel `half`
                    [xl, 0, zl],                  # u = -0.5: column 0
                    [xr, 0, zl],                  # u = W - 0.5: column W, outside
                    [0.1, 0.1, 0],                # zc = 0
                    [0, 0, z_eq],                 # zc - d = tolerance: kept
                    [0, 0, z_above],              # one float above: dropped
                    [np.nan, 0, 1], [0, np.nan, 1], [0, 0, np.nan]], dtype=F32)
    pixels = [(row, half, 1.0), (row, half - 1, 0.0), (row, 0, 3.0), (row, W - 1, 3.0), (row, col, float(t))]
    assert len({(r, c) for r, c, _ in pixels}) == len(pixels) and len(pts) == N_EDGE
    return pts, pixels, [1, 1, 0, 0, 1, 0, 0, 0, 0]


def _case(shape, N, seed=0, lo=(-3.0, -3.0, -1.0), hi=(3.0, 3.0, 4.0)):
    """-> (cam, points [N,3] float32 uniform in the box lo..hi of the first camera's frame - by default one that reaches
    behind the camera -, [(depth [H,W] float32, c2w)] of three frames)."""
    cam = CAMS[shape]
    rng = np.random.default_rng(seed + N)
    pts = (np.asarray(lo) + rng.random((N, 3)) * (np.asarray(hi) - np.asarray(lo))).astype(F32)
    edge, pixels, _ = _edge_points(cam)
    if N >= N_EDGE:
        pts[:N_EDGE] = edge
    frames = []
    for k, c2w in enumerate(_poses()):
        depth = (0.5 + 2.5 * rng.random((cam.H, cam.W))).astype(F32)
        depth[rng.random((cam.H, cam.W)) < 0.1] = 0.0
        if k == 0:
            for r, c, d in pixels:
                depth[r, c] = d
        frames.append((depth, c2w))
    return cam, pts, frames


def _K(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy)


def _reference(cam, pts, frames, repeat=1):
    views = np.zeros(len(pts), np.int32)
    for depth, c2w in frames:
        for _ in range(repeat):
            vr.views_add(views, pts, depth, _K(cam), TRANSFORM @ c2w, TOL)
    return views


def _cull(cam, pts, faces, **kw):
    return evaluation.VisibilityCull(pts, faces, cam, transform=TRANSFORM, tolerance=TOL, device="cuda", **kw)


NO_FACES = np.zeros((0, 3), np.int32)


@pytest.mark.parametrize("shape", sorted(CAMS))
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 100003])
def test_views_match_the_definition(shape, N):
    cam, pts, frames = _case(shape, N)
    cull = _cull(cam, pts, NO_FACES)
    for k, (depth, c2w) in enumerate(frames):
        d = torch.from_numpy(depth).cuda()
        cull.add(d if k % 2 == 0 else d.reshape(cam.H, cam.W, 1), c2w)          # both accepted shapes
    want = _reference(cam, pts, frames)
    assert cull.views.dtype == torch.int32 and cull.frames == 3
    assert torch.equal(cull.views.cpu(), torch.from_numpy(want))
    if N >= 1000:
        assert 0 < int((want > 0).sum()) < N and want.max() <= 3


@pytest.mark.parametrize("shape", sorted(CAMS))
def test_edge_points_at_the_identity_frame(shape):
    cam, pts, frames = _case(shape, 1000)
    _, _, expect = _edge_points(cam)
    cull = _cull(cam, pts, NO_FACES)
    cull.add(torch.from_numpy(frames[0][0]).cuda(), frames[0][1])
    want = _reference(cam, pts, frames[:1])
    assert want[:N_EDGE].tolist() == expect                                      # the definition itself
    assert torch.equal(cull.views.cpu(), torch.from_numpy(want))


def test_the_same_frame_twice_doubles_the_counts():
    cam, pts, frames = _case((48, 64), 1000)
    cull = _cull(cam, pts, NO_FACES)
    for depth, c2w in frames:
        d = torch.from_numpy(depth).cuda()
        cull.add(d, c2w)
        cull.add(d, c2w)
    once = _reference(cam, pts, frames)
    assert cull.frames == 6 and torch.equal(cull.views.cpu(), torch.from_numpy(2 * once))
    assert torch.equal(cull.views.cpu(), torch.from_numpy(_reference(cam, pts, frames, repeat=2)))


def test_empty_inputs():
    cam, pts, frames = _case((17, 23), 65)
    d = torch.from_numpy(frames[0][0]).cuda()
    cull = _cull(cam, np.zeros((0, 3), F32), NO_FACES)
    cull.add(d, frames[0][1])
    v, f = cull.mesh()
    assert cull.views.shape == (0,) and v.shape == (0, 3) and f.shape == (0, 3)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda
    rep = cull.report()
    assert (rep["V"], rep["F"], rep["V_kept"], rep["F_kept"], rep["frames"]) == (0, 0, 0, 0, 1)
    cull = _cull(cam, pts, NO_FACES)                                            # points without faces
    cull.add(d, frames[0][1])
    v, f = cull.mesh()
    assert cull.keep().shape == (0,) and v.shape == (0, 3) and f.shape == (0, 3)
    assert torch.equal(cull.views.cpu(), torch.from_numpy(_reference(cam, pts, frames[:1])))


@pytest.mark.parametrize("any_vertex", [False, True])
@pytest.mark.parametrize("min_views", [1, 3])
def test_keep_faces(any_vertex, min_views):
    rng = np.random.default_rng(7)
    V, F = 5000, 20011
    views = rng.integers(0, 5, V).astype(np.int32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    got = evaluation.visibility_keep_faces(torch.from_numpy(faces).cuda(), torch.from_numpy(views).cuda(), min_views, any_vertex)
    want = vr.keep_faces(faces, views, min_views, any_vertex)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), torch.from_numpy(want))
    assert 0 < int(want.sum()) < F


@pytest.mark.parametrize("any_vertex", [False, True])
def test_mesh_is_cull_mesh(any_vertex):
    cam, pts, frames = _case((48, 64), 1000, lo=(-0.5, -0.5, 0.2), hi=(0.5, 0.5, 1.2))      # most of them in view of all three
    faces = np.random.default_rng(3).integers(0, len(pts), (3001, 3)).astype(np.int32)
    cull = _cull(cam, pts, faces, min_views=2, any_vertex=any_vertex)
    for depth, c2w in frames:
        cull.add(torch.from_numpy(depth).cuda(), c2w)
    views = _reference(cam, pts, frames)
    wv, wf = vr.cull_mesh(pts, faces, views, 2, any_vertex)
    v, f = cull.mesh()
    assert 0 < len(wf) < len(faces)
    assert torch.equal(f.cpu(), torch.from_numpy(wf))
    assert torch.equal(v.cpu().view(torch.int32), torch.from_numpy(wv).view(torch.int32))          # bits: NaN rows included
    rep = cull.report()
    assert (rep["V"], rep["F"], rep["V_kept"], rep["F_kept"]) == (len(pts), len(faces), len(wv), len(wf))
    assert rep["frames"] == 3 and rep["min_views"] == 2 and rep["keep"] == ("any" if any_vertex else "all")
    assert abs(rep["tolerance"] - TOL) < 1e-8 and rep["seconds"] > 0
    # mesh_ops.keep_faces carries colours along when it is given some
    colors = torch.rand(len(pts), 3, device="cuda")
    kv, kf, kc = mesh_ops.keep_faces(cull.vertices, cull.faces, colors, cull.keep())
    used = np.unique(faces[vr.keep_faces(faces, views, 2, any_vertex).astype(bool)])
    assert torch.equal(kf, f) and torch.equal(kc.cpu(), colors.cpu()[torch.from_numpy(used)])


def test_bad_input_raises():
    cam, pts, frames = _case((17, 23), 65)
    depth = torch.from_numpy(frames[0][0])
    with pytest.raises(RuntimeError, match="HIP device"):
        evaluation.VisibilityCull(torch.from_numpy(pts), NO_FACES, cam)
    cull = _cull(cam, pts, NO_FACES)
    with pytest.raises(RuntimeError, match="HIP device"):
        cull.add(depth, np.eye(4))
    with pytest.raises(ValueError, match="contiguous"):
        cull.add(torch.zeros(cam.H, 2 * cam.W, device="cuda")[:, ::2], np.eye(4))
    with pytest.raises(ValueError, match="float32"):
        cull.add(depth.double().cuda(), np.eye(4))
    with pytest.raises(ValueError):
        cull.add(torch.zeros(cam.H + 1, cam.W, device="cuda"), np.eye(4))
    views = torch.zeros(len(pts), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="float32"):
        evaluation.visibility_add(views, torch.from_numpy(pts).double().cuda(), depth.cuda(), _K(cam), np.eye(4), TOL)
    with pytest.raises(RuntimeError, match="HIP device"):
        evaluation.visibility_add(views, torch.from_numpy(pts), depth.cuda(), _K(cam), np.eye(4), TOL)
    with pytest.raises(ValueError):
        evaluation.visibility_add(views, torch.from_numpy(pts).cuda(), depth.cuda(), _K(cam), np.eye(4), -0.01)
    with pytest.raises(ValueError, match="face indices"):
        _cull(cam, pts, np.array([[0, 1, len(pts)]], np.int32))
    with pytest.raises(ValueError, match="min_views"):
        _cull(cam, pts, NO_FACES, min_views=0)
    assert cull.frames == 0 and not cull.views.any()
