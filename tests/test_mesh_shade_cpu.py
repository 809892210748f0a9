"""tests/mesh_shade_reference.py - the definition the colour pass of csrc/mesh_render.hip is held to - against facts: a ramp that
only perspective-correct weights reproduce, a shared edge through pixel centres, an atlas clamped at its borders, blocks of the
bake's layout, inputs that must draw nothing, and the quality case of tests/test_mesh_texture_cpu.py in picture space.  No GPU
(the ABI's refusals launch nothing)."""
import numpy as np
import pytest

from rtg_slam_amd import synth
from tests import mesh_render_reference as rr
from tests import mesh_shade_cases as cases
from tests import mesh_shade_reference as sr
from tests import mesh_texture_reference as tr
from tests import visibility_reference as vr

F32 = np.float32


def _shade(case, source):
    cam = case["cam"]
    kw = {"colors": case["colors"]} if source == "vertex" else {"uv": case["uv"], "texture": case["texture"]}
    out = sr.shade(case["v"], case["f"], cases.face_map(case), cases.K(cam), cam.H, cam.W, case["c2w"],
                   background=case["background"], **kw)
    assert out.dtype == F32 and out.shape == (3, cam.H, cam.W)
    return out


def test_a_ramp_needs_perspective_correct_weights():
    """A quad of two triangles seen at 60 degrees from its normal, 1.7 to 4.3 m deep, its vertex colours linear in the world
    position: the render is that function at the ray-plane intersection (within 1e-5), and the screen-space weights w_k / area
    are not (off by more than 1e-2 somewhere)."""
    case = cases.ramp()
    cam, c2w = case["cam"], case["c2w"]
    n = c2w[:3, 2]
    assert abs(np.degrees(np.arccos(abs(n[2]))) - 60.0) < 1e-9                # the camera's axis against the plane's normal
    fm = cases.face_map(case)
    hit = fm >= 0
    assert 0.2 < hit.mean() < 1.0 and set(np.unique(fm)) == {-1, 0, 1}
    got = _shade(case, "vertex")
    ys, xs = np.meshgrid(np.arange(cam.H, dtype=np.float64), np.arange(cam.W, dtype=np.float64), indexing="ij")
    d = np.stack([(xs - cam.cx) / cam.fx, (ys - cam.cy) / cam.fy, np.ones_like(xs)], -1) @ c2w[:3, :3].T
    t = -c2w[2, 3] / d[..., 2]
    world = c2w[:3, 3] + t[..., None] * d                                     # the ray's point on z = 0
    want = cases.ramp_color(world).transpose(2, 0, 1)
    err = np.abs(got.astype(np.float64) - want)[:, hit].max()
    print("perspective-correct: largest error", err)
    assert err < 1e-5
    for c in range(3):
        assert np.array_equal(got[c][~hit], np.full((~hit).sum(), F32(case["background"][c])))
    # the same pixels with the screen-space weights
    ok, _, fi, (w0, w1, w2) = sr.weights(case["v"], case["f"], fm, cases.K(cam), cam.H, cam.W, c2w)
    assert np.array_equal(ok, hit)
    area = ((w0 + w1) + w2).astype(np.float64)
    col = case["colors"].astype(np.float64)[case["f"][fi]]                   # [H,W,3 corners,3 channels]
    screen = sum((w / area)[..., None] * col[..., k, :] for k, w in enumerate((w0, w1, w2))).transpose(2, 0, 1)
    off = np.abs(screen - want)[:, hit].max()
    print("screen-space: largest error", off)
    assert off > 1e-2


def test_a_shared_edge_through_pixel_centres():
    """Every pixel, the diagonal's included, is shaded with the face the face map names; both windings give one picture."""
    pictures = []
    for flip in (False, True):
        case = cases.shared_edge(flip)
        fm = cases.face_map(case)
        diagonal = [(4 + k, 8 + k) for k in range(33)]
        assert all(fm[r, c] == 0 for r, c in diagonal)                          # equal depth: the lower index
        assert (fm == 1).sum() == 32 * 33 // 2 and (fm == 0).sum() == 33 * 34 // 2
        got = _shade(case, "vertex")
        want = np.where(fm[None] >= 0, cases.PALETTE[np.maximum(fm, 0)].transpose(2, 0, 1), F32(0))
        assert np.array_equal(got, want)
        pictures.append(got)
    assert np.array_equal(pictures[0], pictures[1])
    ys, xs = np.meshgrid(np.arange(cases.HAND.H), np.arange(cases.HAND.W), indexing="ij")
    for flip in (False, True):
        case = cases.shared_edge_linear(flip)
        hit = cases.face_map(case) >= 0
        assert hit.sum() == 33 * 33
        want = np.where(hit[None], np.stack([xs / 64.0, ys / 64.0, np.full(xs.shape, 0.5)]), 0.0).astype(F32)
        assert np.array_equal(_shade(case, "vertex"), want)                      # exact: every weight a multiple of 2^-10


def test_a_two_by_two_atlas_is_clamped_at_its_borders():
    case = cases.atlas_2x2()
    got = _shade(case, "texture")
    tex = cases.ATLAS_2X2.astype(F32) / F32(255)
    for (r, c), (ty, tx) in {(4, 8): (0, 0), (4, 40): (0, 1), (36, 40): (1, 1), (36, 8): (1, 0)}.items():
        assert np.array_equal(got[:, r, c], tex[ty, tx])                         # uv exactly 0 or 1: the corner texel itself
    # tu = (px - 8) / 32: X = 2 tu - 0.5 is clamped to 0 over the first quarter and to 1 over the last
    assert np.array_equal(got[:, 4:37, 8:17], np.repeat(got[:, 4:37, 8:9], 9, axis=2))
    assert np.array_equal(got[:, 4:37, 32:41], np.repeat(got[:, 4:37, 40:41], 9, axis=2))
    assert np.array_equal(got[:, 4:13, 8:41], np.repeat(got[:, 4:5, 8:41], 9, axis=1))
    assert np.array_equal(got[:, 28:37, 8:41], np.repeat(got[:, 36:37, 8:41], 9, axis=1))
    ys, xs = np.meshgrid(np.arange(48, dtype=np.float64), np.arange(64, dtype=np.float64), indexing="ij")
    X, Y = np.clip(2 * (xs - 8) / 32 - 0.5, 0, 1), np.clip(2 * (ys - 4) / 32 - 0.5, 0, 1)
    t64 = cases.ATLAS_2X2.astype(np.float64) / 255
    want = ((1 - Y) * (1 - X))[..., None] * t64[0, 0] + ((1 - Y) * X)[..., None] * t64[0, 1] + \
        (Y * (1 - X))[..., None] * t64[1, 0] + (Y * X)[..., None] * t64[1, 1]
    hit = cases.face_map(case) >= 0
    assert hit.sum() == 33 * 33
    assert np.abs(got.astype(np.float64) - want.transpose(2, 0, 1))[:, hit].max() < 1e-6
    assert not got[:, ~hit].any()
    # a constant atlas renders that constant, at byte / 255
    one = _shade(cases.atlas_2x2(np.full((2, 2, 3), 77, np.uint8)), "texture")
    assert (one[:, hit] == F32(77) / F32(255)).all()


def test_a_fetch_stays_in_its_block():
    """Four faces on the bake's layout of the levels 1, 3, 1, 2 (a 16 x 8 atlas), corners at texel centres: every pixel of a face
    shows the one colour of its block, never the poison around it."""
    case, colours = cases.blocks()
    assert case["texture"].shape == (8, 16, 3) and (case["texture"] == cases.POISON).all(axis=-1).any()
    fm = cases.face_map(case)
    assert set(np.unique(fm)) == {-1, 0, 1, 2, 3}
    got = _shade(case, "texture")
    want = np.where(fm[None] >= 0, (colours.astype(F32) / F32(255))[np.maximum(fm, 0)].transpose(2, 0, 1), F32(0))
    assert np.array_equal(got, want)
    const, _ = cases.blocks((9, 99, 199))
    got = _shade(const, "texture")
    for c, byte in enumerate((9, 99, 199)):
        assert (got[c][fm >= 0] == F32(byte) / F32(255)).all() and not got[c][fm < 0].any()


@pytest.mark.parametrize("name", sorted(cases.nothing_cases()))
def test_nothing_to_draw_gives_the_background(name):
    case = cases.nothing_cases()[name]
    cam = case["cam"]
    if name == "a face across the near plane":
        assert (rr.render(case["v"], case["f"], cases.K(cam), cam.H, cam.W, case["c2w"])[1] == -1).all()
    got = _shade(case, "vertex")
    for c in range(3):
        assert (got[c] == F32(case["background"][c])).all()


def test_shade_wants_exactly_one_source():
    case = cases.ramp()
    cam = case["cam"]
    args = (case["v"], case["f"], cases.face_map(case), cases.K(cam), cam.H, cam.W, case["c2w"])
    for kw in ({}, {"colors": case["colors"], "uv": case["uv"], "texture": case["texture"]}, {"uv": case["uv"]},
               {"texture": case["texture"]}):
        with pytest.raises(ValueError):
            sr.shade(*args, **kw)


def test_the_abi_refuses_before_it_launches():
    """rtgs_mesh_shade returns -1 for every argument set it must not run with; no pointer can be followed, so nothing was
    launched."""
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from rtg_slam_amd import _lib
    lib = _lib.load()
    m = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    bg = (C.c_float * 3)(0, 0, 0)
    one = C.c_void_p(8)                                   # a non-null pointer that is never followed

    def call(V=3, F=1, H=4, W=4, near=0.05, w2c=m, vertices=one, faces=one, face_map=one, colors=None, uv=None, texture=None,
             Ht=2, Wt=2, background=bg, out=one):
        return lib.rtgs_mesh_shade(vertices, V, faces, F, face_map, H, W, 16.0, 16.0, 2.0, 2.0, w2c, near, colors, uv, texture, Ht, Wt,
                                   background, out, None)

    vertex, texture = {"colors": one}, {"uv": one, "texture": one}
    for src in (vertex, texture):
        assert call(F=2 ** 31, **src) == -1 and call(F=-1, **src) == -1 and call(V=-1, **src) == -1
        assert call(H=65536, W=32768, **src) == -1 and call(H=0, **src) == -1 and call(W=-4, **src) == -1
        assert call(near=0.0, **src) == -1 and call(near=-1.0, **src) == -1 and call(near=float("nan"), **src) == -1
        assert call(w2c=None, **src) == -1 and call(face_map=None, **src) == -1 and call(out=None, **src) == -1
        assert call(background=None, **src) == -1
        assert call(vertices=None, **src) == -1 and call(faces=None, **src) == -1 and call(V=0, **src) == -1
    assert call() == -1                                                         # no source
    assert call(colors=one, uv=one, texture=one) == -1                          # both
    assert call(uv=one) == -1 and call(texture=one) == -1                       # half a texture
    assert call(colors=one, uv=one) == -1 and call(colors=one, texture=one) == -1
    side = 16384
    for bad in ({"Ht": 0}, {"Wt": 0}, {"Ht": -1}, {"Ht": side + 1}, {"Wt": side + 1}):
        assert call(**texture, **bad) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the quality case, in picture space
# ---------------------------------------------------------------------------------------------------------------------

PATTERN_SCALE = 24.0                  # tests/test_mesh_texture_cpu.py's pattern: a period of about 0.2 m
QUALITY_TEXTURE, QUALITY_VERTEX = 0.00530, 0.25653                                   # the definition's figures, recorded below


def _quarter_replica():
    c = synth.REPLICA
    return synth.CameraSpec(c.H // 4, c.W // 4, c.fx / 4, c.fy / 4, (c.cx + 0.5) / 4 - 0.5, (c.cy + 0.5) / 4 - 0.5)


def pattern(p):
    """synth.box_room_color's formula with its frequencies scaled up, as a function of the world point -> [..., 3]."""
    p = np.asarray(p, dtype=np.float64)
    s = PATTERN_SCALE
    return 0.5 + 0.35 * np.stack([np.sin(s * (1.3 * p[..., 0] + 0.7 * p[..., 2])), np.cos(s * (1.1 * p[..., 1] - 0.4 * p[..., 0])),
                                  np.sin(s * (0.9 * p[..., 2] + 0.5 * p[..., 1]))], -1)


def pattern_image(cam, c2w, depth):
    """The pattern at the world point every pixel sees, as synth.box_room_color forms that point -> [3,H,W] float32."""
    H, W = cam.H, cam.W
    c2w = np.asarray(c2w, dtype=np.float64)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = np.asarray(depth, dtype=np.float64).reshape(H, W)
    pc = np.stack([(xs - cam.cx) / cam.fx * z, (ys - cam.cy) / cam.fy * z, z], -1)
    return np.ascontiguousarray(pattern(pc @ c2w[:3, :3].T + c2w[:3, 3]).transpose(2, 0, 1)).astype(F32)


def test_quality_a_textured_render_against_a_vertex_coloured_one():
    """The quality case of tests/test_mesh_texture_cpu.py, judged in the picture: the flat room at a cell of 0.5 m (1 008 faces),
    the pattern with a period of about 0.2 m, the six poses of synth.trajectory(6, seed=1, max_rot_deg=60, max_trans=0.1) on a
    quarter-size Replica camera (170 x 300), the atlas baked by mesh_texture_reference.texture_mesh at a texel of 2 cm (2048 x
    2048) from those six views.  The mesh is rendered at the six poses with both sources; over the hit pixels (all 306 000: the
    room is closed), the mean absolute error against pattern_image, recorded from the numpy definition:
        texture source              0.00530
        vertex source               0.25653    (the pattern's own mean deviation: three corners carry nothing of it)
    The texture error must lie below the vertex error and within a quarter of the recorded figure, the vertex error within
    0.01 of its own."""
    cam = _quarter_replica()
    Kc = (cam.fx, cam.fy, cam.cx, cam.cy)
    v, f = vr.box_grid(vr.ROOM_HALF, cell=0.5)
    assert len(f) == 1008
    colors = pattern(v).astype(F32)
    poses, views, depths = [], [], []
    for pose in synth.trajectory(6, seed=1, max_rot_deg=60.0, max_trans=0.1):
        d = synth.box_room_depth(cam, pose, bump=0)[..., 0].numpy()
        poses.append(pose.numpy())
        depths.append(d)
        views.append((pattern_image(cam, pose.numpy(), d), pose.numpy()))
    out = tr.texture_mesh(v, f, colors, Kc, cam.H, cam.W, views, texel=0.02, tolerance=0.02, depths=depths)
    assert (out["layout"]["Wt"], out["layout"]["Ht"]) == (2048, 2048)
    sums = {"vertex": 0.0, "texture": 0.0}
    n = 0
    for (truth, c2w) in views:
        fm = rr.render(v, f.astype(np.int32), Kc, cam.H, cam.W, c2w)[1]
        hit = fm >= 0
        assert hit.all()                                                         # a closed room
        n += 3 * int(hit.sum())
        for name, kw in (("vertex", {"colors": colors}), ("texture", {"uv": out["uv"], "texture": out["image"]})):
            got = sr.shade(v, f, fm, Kc, cam.H, cam.W, c2w, **kw)
            sums[name] += float(np.abs(got.astype(np.float64) - truth.astype(np.float64))[:, hit].sum())
    texture, vertex = sums["texture"] / n, sums["vertex"] / n
    print(f"picture space over {n // 3} pixels: texture {texture:.5f}, vertex colours {vertex:.5f}")
    assert texture < vertex
    assert texture <= 1.25 * QUALITY_TEXTURE
    assert abs(vertex - QUALITY_VERTEX) < 0.01
