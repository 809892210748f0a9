"""The numpy definition of the mesh texture bake (tests/mesh_texture_reference.py) on cases whose answers are known by hand, the
OBJ / MTL / PNG round trip, and the quality case: a texture against three corner colours on a decimated flat room.  No GPU."""
import numpy as np
import torch

from rtg_slam_amd import io_formats as iof, synth
from tests import mesh_texture_reference as tr, visibility_reference as vr

F32 = np.float32
EYE = np.eye(4)


def _quarter_replica():
    c = synth.REPLICA
    return synth.CameraSpec(c.H // 4, c.W // 4, c.fx / 4, c.fy / 4, (c.cx + 0.5) / 4 - 0.5, (c.cy + 0.5) / 4 - 0.5)


def _edge_face(length):
    """A triangle whose longest edge (along x, from the origin) has exactly this float32 length."""
    return [[0, 0, 0], [F32(length), 0, 0], [F32(length) * F32(0.5), F32(length) * F32(0.25), 0]]


def test_levels_at_the_thresholds():
    texel = F32(0.1)
    verts, want_level, want_cap = [], [], []
    for l in range(1, 7):
        t = F32((1 << l) - 1) * texel
        verts += _edge_face(t)                                     # exactly (s - 1) texel: fits level l
        want_level.append(l)
        want_cap.append(0)
        verts += _edge_face(np.nextafter(t, F32(np.inf)))          # one ulp longer: the next level, or capped at 6
        want_level.append(min(l + 1, 6))
        want_cap.append(int(l == 6))
    verts += _edge_face(100.0)                                     # far over the cap
    want_level.append(6)
    want_cap.append(1)
    verts += [[1, 2, 3]] * 3                                       # no extent at all
    want_level.append(1)
    want_cap.append(0)
    verts += [[0, 0, 0], [np.nan, 0, 0], [0, 1, 0]]                # a NaN corner
    want_level.append(1)
    want_cap.append(0)
    verts += [[0, 0, 0], [np.inf, 0, 0], [0, 1, 0]]                # an infinite corner
    want_level.append(1)
    want_cap.append(0)
    v = np.asarray(verts, dtype=F32)
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    levels, capped = tr.face_levels(v, f, texel)
    assert levels.tolist() == want_level and capped.tolist() == want_cap
    # a lower max_level caps earlier
    levels, capped = tr.face_levels(v[:36], f[:12], texel, max_level=3)
    assert levels.tolist() == [min(l, 3) for l in want_level[:12]]
    assert capped.tolist() == [0, 0, 0, 0, 0, 1] + [1] * 6


def _check_packing(levels):
    levels = np.asarray(levels, dtype=np.int32)
    lay = tr.layout(levels)
    Wt, Ht, T = lay["Wt"], lay["Ht"], lay["T"]
    assert T == int((4 ** levels.astype(np.int64)).sum())
    assert Wt == tr.atlas_size(T)[0] and Ht in (Wt, Wt // 2) and Wt * Ht >= T and (Ht == Wt) == (2 * T > Wt * Wt)
    if Wt > 1:
        assert 4 * T > Wt * Wt                                     # no smaller power of four holds T
    owner = np.full((Ht, Wt), -1, dtype=np.int32)
    count = np.zeros((Ht, Wt), dtype=np.int32)
    for face, (l, (x0, y0)) in enumerate(zip(levels, lay["origin"])):
        s = 1 << int(l)
        assert x0 % s == 0 and y0 % s == 0, "origins are aligned to the block size"
        assert 0 <= x0 and x0 + s <= Wt and 0 <= y0 and y0 + s <= Ht, "blocks lie inside the atlas"
        owner[y0:y0 + s, x0:x0 + s] = face
        count[y0:y0 + s, x0:x0 + s] += 1
    assert count.max() <= 1 and int(count.sum()) == T, "blocks are disjoint"
    tf = tr.texel_face(lay)
    assert np.array_equal(tf, owner), "the binary search returns the owner, -1 elsewhere"
    y, x = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    code = tr.morton_encode(x, y)
    assert np.array_equal(tf >= 0, code < T), "the blocks are gap-free up to T"
    # sorted by level descending, stable in the face index
    order = lay["order"]
    key = list(zip((-levels[order]).tolist(), order.tolist()))
    assert key == sorted(key)
    return lay


def test_packing_on_mixed_level_sets():
    half = _check_packing([1, 2, 1, 1, 1])                          # T = 32 = 2^(2 3 - 1): the half-height atlas
    assert (half["T"], half["Wt"], half["Ht"]) == (32, 8, 4)
    full = _check_packing([1, 2, 2, 1, 2, 1, 1])                    # T = 64: fills the square exactly
    assert (full["T"], full["Wt"], full["Ht"]) == (64, 8, 8)
    assert (tr.texel_face(full) >= 0).all()
    one = _check_packing([1])
    assert (one["T"], one["Wt"], one["Ht"]) == (4, 2, 2)
    just_over = _check_packing([2, 2, 1])                           # T = 36 > 32: the full square
    assert (just_over["Wt"], just_over["Ht"]) == (8, 8)
    _check_packing([6, 1, 3, 3, 5, 2, 1, 1, 4, 6, 2])
    rng = np.random.default_rng(5)
    for _ in range(40):
        _check_packing(rng.integers(1, 7, size=int(rng.integers(1, 200))))
    empty = tr.layout(np.zeros(0, dtype=np.int32))
    assert (empty["T"], empty["Wt"], empty["Ht"]) == (0, 1, 1) and tr.texel_face(empty).tolist() == [[-1]]


def test_morton_round_trip():
    x, y = np.meshgrid(np.arange(0, 16384, 37), np.arange(0, 16384, 41))
    code = tr.morton_encode(x, y)
    dx, dy = tr.morton_decode(code)
    assert np.array_equal(dx, x) and np.array_equal(dy, y)
    assert tr.morton_encode(np.array([1, 0, 3]), np.array([0, 1, 3])).tolist() == [1, 2, 15]


def test_mirror_rule():
    for level in (1, 2, 3, 6):
        s = 1 << level
        lay = tr.layout(np.array([level], dtype=np.int32))
        tf = tr.texel_face(lay)
        assert tf.shape == (s, s) and (tf == 0).all()
        a, b = tr.texel_ab(tf, np.array([level]), lay)
        j, i = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
        assert ((a >= 0) & (b >= 0) & (a.astype(np.float64) + b <= 1 + 1e-6)).all(), "every texel maps into the triangle"
        lower = i + j <= s - 1
        assert np.array_equal(a[lower], (i[lower].astype(F32) / F32(s - 1))) and np.array_equal(b[lower], j[lower].astype(F32) / F32(s - 1))
        assert np.array_equal(a[~lower], ((s - 1 - j)[~lower].astype(F32) / F32(s - 1)))
        assert np.array_equal(b[~lower], ((s - 1 - i)[~lower].astype(F32) / F32(s - 1)))
        hyp = i + j == s - 1                                        # the hypotenuse is its own mirror image
        assert np.array_equal((s - 1 - j)[hyp], i[hyp]) and np.array_equal((s - 1 - i)[hyp], j[hyp])
        assert np.allclose(a[hyp].astype(np.float64) + b[hyp], 1.0, atol=1e-6)
        # the texel (i, j) above the hypotenuse and its mirror image below it land on the same surface point
        assert np.array_equal(a[j, i][~lower], a[(s - 1 - i), (s - 1 - j)][~lower])
    v = np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2]], dtype=F32)
    P = tr.texel_points(v, [[0, 1, 2]], tf, a, b)
    assert np.array_equal(P[0, 0], v[0]) and np.array_equal(P[0, s - 1], v[1]) and np.array_equal(P[s - 1, 0], v[2])


CAM = synth.CameraSpec(48, 64, 50.0, 50.0, 31.5, 23.5)
K = (CAM.fx, CAM.fy, CAM.cx, CAM.cy)


def _ramp(H, W):
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([0.1 + 0.01 * x + 0.002 * y, 0.9 - 0.008 * x - 0.004 * y, 0.2 + 0.003 * x + 0.012 * y]).astype(F32)


def _plane(z):
    """The depth map of a wall at camera z: what a closed mesh around the test's triangles would render."""
    return [np.full((CAM.H, CAM.W), z, dtype=F32)]


def _ramp_at(P):
    P = P.astype(np.float64)
    u, v = CAM.fx * P[..., 0] / P[..., 2] + CAM.cx, CAM.fy * P[..., 1] / P[..., 2] + CAM.cy
    return np.stack([0.1 + 0.01 * u + 0.002 * v, 0.9 - 0.008 * u - 0.004 * v, 0.2 + 0.003 * u + 0.012 * v], -1)


def test_a_facing_triangle_reproduces_a_linear_ramp():
    v = np.array([[-0.5, -0.4, 2], [0.6, -0.3, 2], [-0.4, 0.5, 2]], dtype=F32)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    out = tr.texture_mesh(v, f, None, K, CAM.H, CAM.W, [(_ramp(CAM.H, CAM.W), EYE)], texel=0.05, tolerance=0.01,
                          depths=_plane(2.0))
    assert out["levels"].tolist() == [5] and out["capped"].tolist() == [0]           # longest edge 1.27 m: 31 texels of 5 cm
    assert out["texels_assigned"] == 1024 and out["texels_seen"] == 1024
    acc = out["acc"][0]
    P = tr.texel_points(v, f, out["texel_face"], out["a"], out["b"])
    want = _ramp_at(P)
    got = acc[..., :3].astype(np.float64) / acc[..., 3:].astype(np.float64)
    assert np.abs(got - want).max() < 2e-5                          # bilinear sampling is exact on a linear image
    w = 1.0 / P[..., 2].astype(np.float64) ** 2 * ((2.0 / np.linalg.norm(P.astype(np.float64), axis=-1)) ** 2)
    assert np.allclose(acc[..., 3], w, rtol=1e-5)                    # cos^2 / z^2 with the normal along z
    assert np.abs(out["image"].astype(np.float64) / 255 - want).max() <= 0.5 / 255 + 2e-5
    uv = out["uv"][0]
    assert np.array_equal(uv, np.array([[0.5, 0.5], [31.5, 0.5], [0.5, 31.5]], dtype=F32) / F32(32))
    # the other winding gives the same bake
    other = tr.texture_mesh(v, f[:, ::-1], None, K, CAM.H, CAM.W, [(_ramp(CAM.H, CAM.W), EYE)], texel=0.05, tolerance=0.01,
                            depths=_plane(2.0))
    assert other["texels_seen"] == 1024
    # two views add up, in order
    two = tr.texture_mesh(v, f, None, K, CAM.H, CAM.W, [(_ramp(CAM.H, CAM.W), EYE)] * 2, texel=0.05, tolerance=0.01,
                          depths=_plane(2.0) * 2)
    # with the depth rendered from the lone triangle itself the interior is seen; a rim texel whose nearest pixel centre lies
    # outside the silhouette meets a hole there (a closed mesh has a neighbouring face instead)
    own = tr.texture_mesh(v, f, None, K, CAM.H, CAM.W, [(_ramp(CAM.H, CAM.W), EYE)], texel=0.05, tolerance=0.01)
    assert 0.85 * 1024 < own["texels_seen"] < 1024
    inner = (out["a"] > 0.1) & (out["b"] > 0.1) & (out["a"] + out["b"] < 0.9)
    assert (own["flags"][inner] == tr.SEEN).all() and np.array_equal(own["acc"][0][inner], acc[inner])
    assert np.array_equal(two["acc"][0], acc) and np.array_equal(two["acc"][1], acc + acc)
    assert np.array_equal(two["image"], out["image"])


def test_a_hidden_triangle_keeps_its_vertex_colours():
    front = np.array([[-0.5, -0.4, 2], [0.6, -0.3, 2], [-0.4, 0.5, 2]], dtype=np.float64)
    centre = front.mean(0)
    back = (centre + 0.8 * (front - centre)) * 1.5                  # the same triangle, shrunk, on the plane z = 3: fully covered
    v = np.concatenate([front, back]).astype(F32)
    f = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    colors = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.2, 0.4, 0.6], [0.9, 0.1, 0.3], [0.5, 0.7, 0.0]], dtype=F32)
    out = tr.texture_mesh(v, f, colors, K, CAM.H, CAM.W, [(_ramp(CAM.H, CAM.W), EYE)], texel=0.05, tolerance=0.01,
                          depths=_plane(2.0))
    tf, flags = out["texel_face"], out["flags"]
    assert (flags[tf == 0] == tr.SEEN).all() and (flags[tf == 1] == tr.ASSIGNED).all() and (flags[tf < 0] == tr.UNASSIGNED).all()
    assert (out["acc"][0][tf == 1] == 0).all()
    a, b = out["a"][tf == 1].astype(np.float64), out["b"][tf == 1].astype(np.float64)
    c = colors.astype(np.float64)
    want = c[3] + a[:, None] * (c[4] - c[3]) + b[:, None] * (c[5] - c[3])
    assert np.abs(out["image"][tf == 1].astype(np.float64) / 255 - want).max() <= 0.5 / 255 + 1e-6
    assert (out["image"][tf < 0] == 0).all()
    # without colours the fallback is mid grey: floor(0.5 * 255 + 0.5) = 128
    grey = tr.texture_mesh(v, f, None, K, CAM.H, CAM.W, [(_ramp(CAM.H, CAM.W), EYE)], texel=0.05, tolerance=0.01, depths=_plane(2.0))
    assert (grey["image"][tf == 1] == 128).all()
    # the same with the depth rendered from the two triangles themselves: the back one is hidden behind the front one
    own = tr.texture_mesh(v, f, colors, K, CAM.H, CAM.W, [(_ramp(CAM.H, CAM.W), EYE)], texel=0.05, tolerance=0.01)
    assert (own["flags"][tf == 1] == tr.ASSIGNED).all() and (own["flags"][tf == 0] == tr.SEEN).sum() > 0.85 * 1024
    # with the front surface gone the back one is seen
    alone = tr.texture_mesh(v, f[1:], colors, K, CAM.H, CAM.W, [(_ramp(CAM.H, CAM.W), EYE)], texel=0.05, tolerance=0.01,
                            depths=_plane(3.0))
    assert alone["texels_seen"] == alone["texels_assigned"] > 0


def test_a_grazing_triangle_is_skipped():
    # a triangle in the plane x = 0.3 in front of the camera: every ray meets it at a cosine of about 0.3 / 2 = 0.15 or less
    v = np.array([[0.3, -0.2, 1.8], [0.3, 0.2, 1.8], [0.3, 0.0, 2.4]], dtype=F32)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    P = v.astype(np.float64)
    assert (np.abs(P[:, 0]) / np.linalg.norm(P, axis=1) < 0.2).all()
    depth = [np.full((CAM.H, CAM.W), 0.1, dtype=F32)]               # with a tolerance of 100 m the depth test passes everywhere
    views = [(_ramp(CAM.H, CAM.W), EYE)]
    out = tr.texture_mesh(v, f, None, K, CAM.H, CAM.W, views, texel=0.05, tolerance=100.0, depths=depth)
    assert out["texels_seen"] == 0 and out["texels_assigned"] > 0 and (out["acc"][0] == 0).all()
    loose = tr.texture_mesh(v, f, None, K, CAM.H, CAM.W, views, texel=0.05, tolerance=100.0, min_cos=0.0, depths=depth)
    assert loose["texels_seen"] == loose["texels_assigned"]
    # behind the camera, outside the image, in a depth hole: nothing
    behind = tr.texture_mesh(v * F32(-1), f, None, K, CAM.H, CAM.W, views, texel=0.05, tolerance=100.0, min_cos=0.0, depths=depth)
    assert behind["texels_seen"] == 0
    aside = tr.texture_mesh(v + F32([30, 0, 0]), f, None, K, CAM.H, CAM.W, views, texel=0.05, tolerance=100.0, min_cos=0.0, depths=depth)
    assert aside["texels_seen"] == 0
    hole = tr.texture_mesh(v, f, None, K, CAM.H, CAM.W, views, texel=0.05, tolerance=100.0, min_cos=0.0,
                           depths=[np.zeros((CAM.H, CAM.W), dtype=F32)])
    assert hole["texels_seen"] == 0


def test_textured_obj_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    v = rng.normal(size=(7, 3)).astype(F32)
    f = rng.integers(0, 7, size=(5, 3)).astype(np.int32)
    levels = np.array([3, 1, 2, 2, 1], dtype=np.int32)
    lay = tr.layout(levels)
    uv = tr.face_uv(lay, levels)
    assert uv.min() > 0 and uv.max() < 1
    image = rng.integers(0, 256, size=(lay["Ht"], lay["Wt"], 3)).astype(np.uint8)
    nrm = rng.normal(size=(7, 3)).astype(F32)
    for normals in (None, nrm):
        path = str(tmp_path / "m.obj")
        iof.save_textured_obj(path, v, f, uv, image, normals, image_name="tex.png")
        assert (tmp_path / "m.mtl").is_file() and (tmp_path / "tex.png").is_file()
        text = open(path).read().split("\n")
        assert text[0] == "mtllib m.mtl" and text[1] == "usemtl textured"
        assert sum(l.startswith("vt ") for l in text) == 15 and sum(l.startswith("vn ") for l in text) == (0 if normals is None else 7)
        first = [l for l in text if l.startswith("f ")][0]
        assert first == (f"f {f[0, 0] + 1}/1 {f[0, 1] + 1}/2 {f[0, 2] + 1}/3" if normals is None else
                         f"f {f[0, 0] + 1}/1/{f[0, 0] + 1} {f[0, 1] + 1}/2/{f[0, 1] + 1} {f[0, 2] + 1}/3/{f[0, 2] + 1}")
        vt0 = [float(x) for x in [l for l in text if l.startswith("vt ")][0].split()[1:]]
        assert vt0 == [float(uv[0, 0, 0]), 1.0 - float(uv[0, 0, 1])]             # v = 1 - y / Ht
        assert "map_Kd tex.png" in open(str(tmp_path / "m.mtl")).read()
        v2, f2, uv2, image2 = iof.load_textured_obj(path)
        assert v2.dtype == F32 and np.array_equal(v2, v) and f2.dtype == np.int32 and np.array_equal(f2, f)
        assert uv2.dtype == F32 and np.array_equal(uv2, uv) and image2.dtype == np.uint8 and np.array_equal(image2, image)
    iof.save_textured_obj(str(tmp_path / "d.obj"), torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(uv), torch.from_numpy(image))
    assert (tmp_path / "d.png").is_file() and np.array_equal(iof.load_textured_obj(str(tmp_path / "d.obj"))[3], image)


# ---------------------------------------------------------------------------------------------------------------------
# the quality case
# ---------------------------------------------------------------------------------------------------------------------

PATTERN_SCALE = 24.0                  # synth.box_room_color's frequencies times this: a period of about 0.2 m
QUALITY_BAKED, QUALITY_VERTEX = 0.00554, 0.2557                                  # the reference's figures, recorded below


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


def test_quality_a_texture_against_three_corner_colours():
    """The flat room at a cell of 0.5 m (1 008 faces, what a decimation leaves of a wall), a pattern with a period of about
    0.2 m, six poses of synth.trajectory(6, seed=1, max_rot_deg=60, max_trans=0.1) on a quarter-size Replica camera (170 x
    300), depth from synth.box_room_depth(bump=0), a texel of 2 cm (level 6 everywhere: a 2048 x 2048 atlas).  Over the seen
    texels, the mean absolute error against the pattern at the texel's point, recorded from this reference:
        baked texture               0.00554
        vertex-colour blend         0.2557     (the pattern's own mean deviation: three corners carry nothing of it)
        seen share                  0.564
    The baked error must lie below the vertex-colour error and within a quarter of the recorded figure."""
    cam = _quarter_replica()
    v, f = vr.box_grid(vr.ROOM_HALF, cell=0.5)
    assert len(f) == 1008
    colors = pattern(v).astype(F32)
    views, depths = [], []
    for pose in synth.trajectory(6, seed=1, max_rot_deg=60.0, max_trans=0.1):
        d = synth.box_room_depth(cam, pose, bump=0)[..., 0].numpy()
        depths.append(d)
        views.append((pattern_image(cam, pose.numpy(), d), pose.numpy()))
    out = tr.texture_mesh(v, f, colors, (cam.fx, cam.fy, cam.cx, cam.cy), cam.H, cam.W, views, texel=0.02, tolerance=0.02, depths=depths)
    assert (out["layout"]["Wt"], out["layout"]["Ht"]) == (2048, 2048) and (out["levels"] == 6).all() and out["capped"].sum() == 0
    seen = out["flags"] == tr.SEEN
    share = out["texels_seen"] / out["texels_assigned"]
    truth = pattern(tr.texel_points(v, f, out["texel_face"], out["a"], out["b"])[seen])
    baked = float(np.abs(out["image"][seen].astype(np.float64) / 255 - truth).mean())
    t = f[out["texel_face"][seen]]
    blend = tr._blend(colors[t[:, 0]], colors[t[:, 1]], colors[t[:, 2]], out["a"][seen], out["b"][seen])
    vertex = float(np.abs(blend.astype(np.float64) - truth).mean())
    print(f"seen share {share:.4f}, baked {baked:.5f}, vertex colours {vertex:.5f}")
    assert share >= 0.5
    assert baked < vertex
    assert baked <= 1.25 * QUALITY_BAKED
    assert abs(vertex - QUALITY_VERTEX) < 0.01
