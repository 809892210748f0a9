"""The colour pass of csrc/mesh_render.hip (rtgs_mesh_shade), evaluation.MeshRenderer.render_color and mesh_color_metrics against
the numpy definition (tests/mesh_shade_reference.py): bit for bit, so every picture is compared with torch.equal."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from rtg_slam_amd import _lib, evaluation, synth
from tests import mesh_render_reference as rr
from tests import mesh_shade_cases as cases
from tests import mesh_shade_reference as sr
from tests import visibility_reference as vr
from tests.tsdf_reference import w2c_from_c2w

pytestmark = pytest.mark.gpu
F32 = np.float32
# a mesh frame that is not the stream's (tests/test_mesh_render_gpu.py): TRANSFORM @ POSE0 is the identity exactly
TRANSFORM = np.array([[0, -1, 0, 0.5], [1, 0, 0, -0.25], [0, 0, 1, 2.0], [0, 0, 0, 1]], dtype=np.float64)
POSE0 = np.array([[0, 1, 0, 0.25], [-1, 0, 0, 0.5], [0, 0, 1, -2.0], [0, 0, 0, 1]], dtype=np.float64)
ODD = synth.CameraSpec(61, 97, 80.5, 75.25, 48.25, 30.75)                   # 97 columns: a row ends inside its second wave
ROOM = synth.CameraSpec(120, 160, 151.25, 138.5, 79.25, 60.75)
BG = (0.25, 0.5, 0.75)


def _K(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy)


def _poses():
    inv_t = np.linalg.inv(TRANSFORM)
    return [POSE0, inv_t @ synth.look_at_pose(seed=5, max_angle_deg=25.0, max_trans=0.4).numpy()]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(got, want):
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and want.dtype == F32
    assert torch.equal(_bits(got), torch.from_numpy(np.ascontiguousarray(want)).view(torch.int32))


def _sources(colors, uv, texture):
    out = []
    if colors is not None:
        out.append(("vertex", {"colors": colors}))
    if uv is not None:
        out.append(("texture", {"uv": uv, "texture": texture}))
    return out


def _check(v, f, cam, c2w_list, colors=None, uv=None, texture=None, transform=None, background=BG):
    """render_color at every pose, both sources where given, against the definition; -> the renderer."""
    T = np.eye(4) if transform is None else transform
    r = evaluation.MeshRenderer(v, f, cam, transform=transform, device="cuda", colors=colors, uv=uv, texture=texture)
    for c2w in c2w_list:
        want_depth, want_face = rr.render(v, f, _K(cam), cam.H, cam.W, T @ c2w)
        for source, kw in _sources(colors, uv, texture):
            want = sr.shade(v, f, want_face, _K(cam), cam.H, cam.W, T @ c2w, background=background, **kw)
            color, depth, face = r.render_color(c2w, source=source, background=background)
            assert color.shape == (3, cam.H, cam.W) and face.dtype == torch.int32
            assert torch.equal(face.cpu(), torch.from_numpy(want_face)) and torch.equal(_bits(depth), torch.from_numpy(want_depth).view(torch.int32))
            _same(color, want)
    return r


def _abi_shade(case, out=None):
    """rtgs_mesh_shade itself on a face map of the caller's choosing -> ([3,H,W] tensor, return code)."""
    cam = case["cam"]
    dev = torch.device("cuda")
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt).contiguous()
    v, f = up(case["v"], torch.float32), up(case["f"], torch.int32)
    fm = up(cases.face_map(case), torch.int32)
    colors, uv, texture = up(case["colors"], torch.float32), up(case["uv"], torch.float32), up(case["texture"], torch.uint8)
    if out is None:
        out = torch.full((3, cam.H, cam.W), -7.0, dtype=torch.float32, device=dev)
    keep = (v, f, fm, colors, uv, texture)
    p = lambda t: C.c_void_p(None) if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
    m = np.ascontiguousarray(w2c_from_c2w(case["c2w"]).reshape(-1)[:12])
    Ht, Wt = (1, 1) if texture is None else texture.shape[:2]
    rc = _lib.load().rtgs_mesh_shade(p(v), int(v.shape[0]), p(f), int(f.shape[0]), p(fm), cam.H, cam.W, *(float(F32(k)) for k in _K(cam)),
                                     (C.c_float * 12)(*m.tolist()), float(F32(rr.NEAR)), p(colors), p(uv), p(texture), int(Ht), int(Wt),
                                     (C.c_float * 3)(*case["background"]), C.c_void_p(out.data_ptr()),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    del keep
    return out, rc


@pytest.mark.parametrize("name", sorted(cases.hand_cases()))
def test_hand_made_cases(name):
    case = cases.hand_cases()[name]
    cam = case["cam"]
    assert (cam.W, cam.H) == (64, 48)
    if case["face_map"] is None:
        _check(case["v"], case["f"], cam, [case["c2w"]], case["colors"], case["uv"], case["texture"], background=case["background"])
        return
    # a face map the rasteriser would not have made: the kernel itself, which must not read out of bounds
    want = sr.shade(case["v"], case["f"], case["face_map"], _K(cam), cam.H, cam.W, case["c2w"], colors=case["colors"],
                    background=case["background"])
    got, rc = _abi_shade(case)
    assert rc == 0
    _same(got, want)


@functools.lru_cache(maxsize=None)
def _soup():
    """300 triangles on 300 vertices (tests/test_mesh_render_gpu.py's soup: subpixel faces, faces of a few pixels, faces larger
    than the picture, faces across the near plane, both windings), vertex colours past 0..1 so that the clamp works, texture
    coordinates past 0..1 so that the atlas's borders do, a 37 x 23 atlas."""
    from tests.test_mesh_render_gpu import _soup as soup
    v, f = soup(300)
    rng = np.random.default_rng(41)
    colors = (rng.random((len(v), 3)) * 1.4 - 0.2).astype(F32)
    uv = (rng.random((len(f), 3, 2)) * 1.2 - 0.1).astype(F32)
    texture = rng.integers(0, 256, (23, 37, 3)).astype(np.uint8)
    return v, f, colors, uv, texture


def test_a_soup_at_97_by_61():
    v, f, colors, uv, texture = _soup()
    for c2w in _poses():
        depth, face = rr.render(v, f, _K(ODD), ODD.H, ODD.W, TRANSFORM @ c2w)
        assert (face >= 0).any() and (face < 0).any() and len(np.unique(face)) > 4
    # both rasteriser paths: boxes of at most 16 pixels by a thread, larger ones by a wave
    u, w, _, usable = rr.project(v, _K(ODD), TRANSFORM @ _poses()[0])
    box = (np.ptp(u[f], axis=1) + 1) * (np.ptp(w[f], axis=1) + 1)
    seen = usable[f].all(axis=1)
    assert (box[seen] <= 16).any() and (box[seen] > 64).any()
    r = _check(v, f, ODD, _poses(), colors, uv, texture, transform=TRANSFORM)
    assert r.renders == 4 and r.seconds > 0
    # two runs are bit-equal
    a = r.render_color(_poses()[1], "texture", BG)
    b = r.render_color(_poses()[1], "texture", BG)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    # render() does not know about the colours, and render_color returns its maps
    plain = evaluation.MeshRenderer(v, f, ODD, transform=TRANSFORM, device="cuda")
    for c2w in _poses():
        d0, f0 = plain.render(c2w)
        d1, f1 = r.render(c2w)
        _, d2, f2 = r.render_color(c2w, "vertex")
        assert torch.equal(_bits(d0), _bits(d1)) and torch.equal(f0, f1) and torch.equal(_bits(d0), _bits(d2)) and torch.equal(f0, f2)


def test_the_wall_grid_in_another_frame():
    gv, gf = vr.box_grid(vr.ROOM_HALF)                                          # 10 cm cells
    rng = np.random.default_rng(43)
    colors = rng.random((len(gv), 3)).astype(F32)
    uv = rng.random((len(gf), 3, 2)).astype(F32)
    texture = rng.integers(0, 256, (64, 128, 3)).astype(np.uint8)
    assert not np.array_equal(TRANSFORM, np.eye(4))
    _check(gv, gf, ROOM, _poses()[1:], colors, uv, texture, transform=TRANSFORM)


def test_nan_vertices_and_faces_behind_the_camera():
    from tests.test_mesh_render_gpu import _soup as soup
    v, f = soup(257)
    n = len(v)
    extra_v = np.array([[0, 0, 1], [0.5, 0.5, 1.5], [1, 1, 2], [np.nan, 0, 1], [0, np.nan, 1], [0, 0, np.nan], [np.inf, 0, 1],
                        [0.2, 0.1, -1.0], [0.4, 0.3, -2.0], [0.1, 0.5, -1.5]], F32)
    extra_f = np.array([[n, n + 1, n + 2], [n + 3, n, n + 2], [n, n + 4, n + 2], [n, n + 1, n + 5], [n + 6, n, n + 2],
                        [n + 7, n + 8, n + 9], [n, n + 1, n + 7]], np.int32)
    v2, f2 = np.concatenate([v, extra_v]), np.concatenate([extra_f, f])
    rng = np.random.default_rng(47)
    colors = rng.random((len(v2), 3)).astype(F32)
    colors[n + 3] = np.nan                                                       # a NaN colour is clamped to 0 where it shows
    uv = rng.random((len(f2), 3, 2)).astype(F32)
    uv[0] = np.nan                                                               # NaN texture coordinates fetch texel (0, 0)
    texture = rng.integers(0, 256, (23, 37, 3)).astype(np.uint8)
    _check(v2, f2, ODD, _poses(), colors, uv, texture, transform=TRANSFORM)


def test_one_pixel_and_one_texel():
    tri = np.array([[-1, -1, 2], [3, -1, 2], [-1, 3, 2]], F32)
    f = np.array([[0, 1, 2]], np.int32)
    colors = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    uv = np.array([[[0.1, 0.2], [0.9, 0.3], [0.4, 0.8]]], F32)
    texture = np.random.default_rng(3).integers(0, 256, (5, 3, 3)).astype(np.uint8)
    one = synth.CameraSpec(1, 1, 1.0, 1.0, 0.0, 0.0)
    r = _check(tri, f, one, [np.eye(4)], colors, uv, texture)
    assert int(r.render_color(np.eye(4), "vertex")[2][0, 0]) == 0
    texel = np.array([[[12, 130, 251]]], np.uint8)
    tri = np.array(cases.QUAD[:3], F32)                                          # a part of the 64 x 48 picture
    r = _check(tri, f, cases.HAND, [np.eye(4)], None, uv, texel)
    color, _, face = r.render_color(np.eye(4), "texture")
    hit = face >= 0
    assert hit.any() and not hit.all()
    for c in range(3):
        assert (color[c][hit].cpu().numpy() == F32(texel[0, 0, c]) / F32(255)).all() and not color[c][~hit].any()
    # a mesh of no faces is the background
    empty = _check(tri, np.zeros((0, 3), np.int32), cases.HAND, [np.eye(4)], colors, np.zeros((0, 3, 2), F32), texel)
    assert (empty.render_color(np.eye(4), "texture", BG)[0][1] == 0.5).all()


def test_bad_input_raises():
    v, f, colors, uv, texture = _soup()
    make = lambda **kw: evaluation.MeshRenderer(v, f, ODD, device="cuda", **kw)
    for kw, word in (({"colors": colors[:-1]}, "colors"), ({"colors": colors[:, :2]}, "colors"),
                     ({"colors": (colors * 255).astype(np.uint8)}, "colors"),
                     ({"uv": uv[:-1], "texture": texture}, "uv"), ({"uv": uv.reshape(-1, 6), "texture": texture}, "uv"),
                     ({"uv": uv.astype(np.int32), "texture": texture}, "uv"),
                     ({"uv": uv, "texture": texture.astype(F32)}, "texture"), ({"uv": uv, "texture": texture[..., :2]}, "texture"),
                     ({"uv": uv, "texture": texture[..., 0]}, "texture"), ({"uv": uv, "texture": texture[:0]}, "texture"),
                     ({"uv": uv}, "texture"), ({"texture": texture}, "uv")):
        with pytest.raises(ValueError, match=word):
            make(**kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        make(colors=torch.from_numpy(colors))
    both = make(colors=colors, uv=uv, texture=texture)
    with pytest.raises(ValueError, match="source"):
        both.render_color(POSE0, source="normals")
    with pytest.raises(ValueError, match="4x4"):
        both.render_color(np.eye(3))
    with pytest.raises(ValueError, match="background"):
        both.render_color(POSE0, background=(0, 0))
    with pytest.raises(ValueError, match="colors"):
        make(uv=uv, texture=texture).render_color(POSE0, source="vertex")
    with pytest.raises(ValueError, match="uv and texture"):
        make(colors=colors).render_color(POSE0, source="texture")
    with pytest.raises(ValueError, match="uv and texture"):
        make().render_color(POSE0, source="texture")
    assert both.renders == 0 and both.seconds == 0.0


def test_the_abi_refuses_and_leaves_out_alone():
    base = cases.ramp()
    marked = torch.full((3, 48, 64), -7.0, dtype=torch.float32, device="cuda")
    vertex = dict(base, uv=None, texture=None)
    textured = dict(base, colors=None)
    assert _abi_shade(vertex, marked.clone())[1] == 0 and _abi_shade(textured, marked.clone())[1] == 0
    refused = [dict(base),                                                       # both sources
               dict(base, colors=None, uv=None, texture=None),                   # none
               dict(base, colors=None, texture=None), dict(base, colors=None, uv=None),
               dict(base, texture=None), dict(base, uv=None),                    # colours and half a texture
               dict(vertex, v=np.zeros((0, 3), F32), face_map=np.zeros((48, 64), np.int32)),      # faces and no vertices
               dict(vertex, cam=synth.CameraSpec(0, 64, 64.0, 64.0, 32.0, 24.0), face_map=np.zeros((1, 1), np.int32))]
    for case in refused:
        out = marked.clone()
        _, rc = _abi_shade(case, out)
        assert rc == -1 and torch.equal(out, marked)
    lib = _lib.load()
    one = C.c_void_p(marked.data_ptr())                                          # a live pointer: nothing may be written through it
    m, bg = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), (C.c_float * 3)(1, 1, 1)
    call = lambda Ht=2, Wt=2, near=0.05, F=1, H=4, W=4: lib.rtgs_mesh_shade(one, 3, one, F, one, H, W, 16.0, 16.0, 2.0, 2.0, m, near, None, one,
                                                                            one, Ht, Wt, bg, one, None)
    for kw in ({"Ht": 0}, {"Wt": 0}, {"Ht": 16385}, {"Wt": 16385}, {"near": 0.0}, {"near": float("nan")}, {"F": 2 ** 31},
               {"H": 65536, "W": 32768}):
        assert call(**kw) == -1
    torch.cuda.synchronize()
    assert (marked == -7.0).all()


def _numpy_metrics(color, gt, face):
    c, g = color.astype(np.float64), gt.astype(np.float64)
    psnr = float(np.mean([20.0 * np.log10(1.0 / np.sqrt(((c[k] - g[k]) ** 2).mean())) for k in range(3)]))
    hit = face >= 0
    diff = np.abs(color - gt)
    assert diff.dtype == F32
    n = int(hit.sum())
    return {"mesh_hit_ratio": n / face.size, "mesh_psnr": psnr, "mesh_color_l1": float(np.abs(c - g).mean()),
            "mesh_color_l1_hit": float(diff[:, hit].astype(np.float64).sum()) / (3 * n) if n else 0.0}


def test_mesh_color_metrics():
    rng = np.random.default_rng(53)
    H, W = 180, 200
    color, gt = rng.random((3, H, W)).astype(F32), rng.random((3, H, W)).astype(F32)
    face = rng.integers(-1, 5, (H, W)).astype(np.int32)
    face[40:90, 30:130] = -1                                                     # a hole of 5 000 pixels, and the scattered -1
    color[:, face < 0] = 0
    dev = lambda a: torch.from_numpy(a).cuda()
    got = evaluation.mesh_color_metrics(dev(color), dev(gt), dev(face))
    want = _numpy_metrics(color, gt, face)
    assert set(got) == set(want) | {"mesh_ssim"}
    assert got["mesh_hit_ratio"] == want["mesh_hit_ratio"] and 0.5 < got["mesh_hit_ratio"] < 0.9
    # float32 pictures, sums in float64: what is left is the rounding of one float32 difference per pixel, 6e-8 relative
    for k in ("mesh_psnr", "mesh_color_l1", "mesh_color_l1_hit"):
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), k
    zero = torch.zeros(H, W, device="cuda")
    whole = evaluation.picture_metrics(dev(color), dev(gt), zero, zero, zero.int(), 0.0, 1.0, True).cpu().tolist()
    assert got["mesh_ssim"] == whole[evaluation.OUT_MS_SSIM] and got["mesh_psnr"] == whole[evaluation.OUT_PSNR]
    # a small picture, without MS-SSIM; a known hole
    h, w = 6, 10
    color, gt = rng.random((3, h, w)).astype(F32), rng.random((3, h, w)).astype(F32)
    face = np.zeros((h, w), np.int32)
    face[1:3, 2:7] = -1
    with pytest.raises(ValueError, match="MS-SSIM"):
        evaluation.mesh_color_metrics(dev(color), dev(gt), dev(face))
    got = evaluation.mesh_color_metrics(dev(color), dev(gt), dev(face), with_ms_ssim=False)
    want = _numpy_metrics(color, gt, face)
    assert got["mesh_ssim"] is None and got["mesh_hit_ratio"] == 50 / 60
    for k in ("mesh_psnr", "mesh_color_l1", "mesh_color_l1_hit"):
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), k
    none = evaluation.mesh_color_metrics(dev(color), dev(gt), dev(face * 0 - 1), with_ms_ssim=False)
    assert none["mesh_hit_ratio"] == 0.0 and none["mesh_color_l1_hit"] == 0.0
    with pytest.raises(ValueError, match="float32"):
        evaluation.mesh_color_metrics(dev(color).double(), dev(gt), dev(face), with_ms_ssim=False)
    with pytest.raises(ValueError, match="do not fit"):
        evaluation.mesh_color_metrics(dev(color), dev(gt), dev(face[:-1]), with_ms_ssim=False)
