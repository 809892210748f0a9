"""The definition of the point-to-mesh distance (tests/mesh_distance_reference.py) against known answers.  No GPU."""
import numpy as np

from tests import mesh_distance_reference as ref

F32 = np.float32
A, B, C = F32([0, 0, 0]), F32([4, 0, 0]), F32([0, 4, 0])          # an axis-aligned face with power-of-two coordinates
U = 2.0 ** -24

# The bound on |sqrt(d2) - d64| for coordinates |x| <= 8, d64 the independent float64 closest point of closest_point_f64.
# Downwards it is derived: every candidate of pair_d2 is the distance to a point of the face, evaluated with a rounding of at most
# eta = 2^-20 (P + 4 M) = 2^-20 * 40 = 3.8e-5 ("mesh distance", step 1), so sqrt(d2) >= d64 - eta.  Upwards no tight
# bound follows from the unit round-off alone: the interior candidate's barycentrics carry the conditioning of the face, and a
# random soup has needles.  So, as the issue allows, the largest deviation over this file's seeded inputs was measured -
# MEASURED below - and the bound is 4 x that; it lies below eta, so the derived side holds with it too.
MEASURED = 3.03e-6                                                # a few ulps of the largest distance, 13.9
BOUND = 4 * MEASURED


def _d2(p, a=A, b=B, c=C, idx=(0, 1, 2)):
    return ref.pair_d2(F32(p), a, b, c, *idx)


def test_corner_edge_interior_are_zero():
    for p in (A, B, C, [2, 0, 0], [0, 1, 0], [2, 2, 0], [1, 1, 0], [0.5, 3, 0]):
        assert _d2(p) == 0 and _d2(p).dtype == F32
    # bit-equal to a corner of a face in general position
    rng = np.random.default_rng(0)
    for _ in range(200):
        a, b, c = (rng.uniform(-8, 8, 3).astype(F32) for _ in range(3))
        for p in (a, b, c):
            for idx in ((0, 1, 2), (2, 1, 0), (5, 3, 4)):
                assert ref.pair_d2(p, a, b, c, *idx) == 0


def test_power_of_two_heights_are_exact():
    for e in range(-20, 11):                                       # legs along the axes from corner a: every height
        h = F32(2.0 ** e)
        for x, y in ((1, 1), (0.3, 0.7), (3.1, 0.2), (0.001, 0.002)):
            for s in (1, -1):
                assert _d2([x, y, s * h]) == h * h, (e, x, y)
    # other axis-aligned faces (no right angle at a; another plane), heights from extent / 64 up
    for a, b, c in ((F32([0, 0, 1]), F32([4, 0, 1]), F32([2, 2, 1])), (F32([2, 2, 0]), F32([0, 0, 0]), F32([4, 0, 0])),
                    (F32([1, 0, 0]), F32([1, 4, 0]), F32([1, 2, 2]))):
        centre = (a.astype(np.float64) + b + c) / 3
        axis = int(np.argmax(np.all([a == b, b == c], axis=0)))
        for e in range(-4, 11):
            h = F32(2.0 ** e)
            for off in ((0, 0, 0), (0.11, 0.07, 0.05)):
                p = centre + np.array(off) * (np.arange(3) != axis)
                p[axis] = float(a[axis]) + float(h)
                assert ref.pair_d2(F32(p), a, b, c) == h * h, (e, a, b, c)


def test_seven_regions_match_the_closed_form():
    for h in (0.0, 0.5, 3.0):
        cases = {"interior": ((1, 1), 0.0), "corner a": ((-1, -2), 5.0), "corner b": ((6, -1), 5.0), "corner c": ((-1, 6), 5.0),
                 "edge ab": ((2, -3), 9.0), "edge ca": ((-3, 2), 9.0), "edge bc": ((4, 4), 8.0)}
        for name, ((x, y), plane2) in cases.items():
            want = plane2 + h * h
            for idx in ((0, 1, 2), (2, 0, 1)):
                got = float(_d2([x, y, h], idx=idx))
                assert abs(got - want) <= 8 * U * want, (name, h, got, want)
            assert abs(ref.distance_f64([x, y, h], A, B, C) ** 2 - want) < 1e-12, name


def test_degenerate_faces_are_finite():
    rng = np.random.default_rng(1)
    for _ in range(100):
        a, b = rng.uniform(-8, 8, 3).astype(F32), rng.uniform(-8, 8, 3).astype(F32)
        mid = (F32(0.5) * (a + b)).astype(F32)
        p = rng.uniform(-8, 8, 3).astype(F32)
        seg64 = ref.distance_f64(p, a, b, b)
        for tri in ((a, a, b), (a, b, b), (a, b, a), (a, a, a), (a, mid, b), (a, b, (a + (b - a) * F32(3)).astype(F32))):
            d = ref.pair_d2(p, *tri)
            assert np.isfinite(d) and d >= 0
        assert abs(np.sqrt(float(ref.pair_d2(p, a, a, a))) - np.linalg.norm(p.astype(np.float64) - a)) < 1e-5
        assert abs(np.sqrt(float(ref.pair_d2(p, a, a, b))) - seg64) < 1e-5
    # the largest coordinates MeshDistance accepts
    big = F32(ref.MAX_COORD)
    for p in ([big, -big, big], [0, 0, 0], [-big, -big, -big]):
        for tri in ((F32([big, big, big]), F32([-big, big, -big]), F32([big, -big, -big])), (A, B, C), (A, A, A)):
            assert np.isfinite(ref.pair_d2(F32(p), *tri))


def test_shared_edge_and_duplicates_take_the_lower_index():
    v, f = ref.hand_made()
    pts = F32([[0.5, 0.5, 0], [0.5, 0.5, 0.25], [0.75, 0.25, 2], [0.25, 0.25, 0], [1, 1, 0.5]])
    d2, face = ref.nearest(pts, v, f)
    # the diagonal 1-2 belongs to faces 0, 1, 2, 3 and 8; faces 0, 2 and 3 are one triangle; 1 and 8 another
    assert face.tolist() == [0, 0, 0, 0, 1] and d2.tolist() == [0, 0.0625, 4, 0, 0.25]
    # the same bits from both faces of the shared edge, so the order of the faces decides
    swapped = f.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    d2s, faces = ref.nearest(pts[:3], v, swapped)
    assert faces.tolist() == [0, 0, 0] and np.array_equal(d2s, d2[:3])
    lv, lf = ref.lattice(4, 0.25)
    lp = ref.lattice_points(4, 0.25)
    ld2, lface = ref.nearest(lp, lv, lf)
    assert np.array_equal(ld2, lp[:, 2] * lp[:, 2])
    for p, k in zip(lp, lface):                                    # no lower face is as near
        assert k == min(i for i in range(len(lf)) if ref.pair_d2(p, *lv[lf[i]], *lf[i]) == p[2] * p[2])


def test_non_finite_points():
    v, f = ref.hand_made()
    pts = F32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.25, 0.25, 1]])
    d2, face = ref.nearest(pts, v, f)
    assert np.isinf(d2[:3]).all() and (d2[:3] > 0).all() and face.tolist() == [-1, -1, -1, 0] and d2[3] == 1


def test_hit_normals():
    v, f = ref.hand_made()
    n = ref.face_unit_normals(v, f)
    assert n.dtype == F32 and n[0].tolist() == [0, 0, 1] and n[3].tolist() == [0, 0, -1]
    assert not n[4].any() and not n[5].any() and not n[6].any()       # the three degenerate kinds
    hit = ref.hit_normals(v, f, np.array([0, -1, 3, 5]))
    assert hit.tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, -1], [0, 0, 0]]
    s, cnt = ref.normal_consistency(hit, ref.hit_normals(v, f, np.array([3, 0, 3, 0])))
    assert (s, cnt) == (2.0, 2)


def test_soup_against_float64():
    worst = 0.0
    for F, seed in ((1, 0), (64, 1), (257, 2), (2000, 3)):
        v, f = ref.soup(F, seed, box=8.0)
        pts = ref.soup_points(v, f, 512, seed + 10)[:384]            # inside, on faces, outside: |coordinate| <= 8 + extent / 2
        pts = np.clip(pts, -8, 8)
        d2, face = ref.nearest(pts, v, f)
        for p, d, k in zip(pts[::3], d2[::3], face[::3]):
            d64 = min(ref.distance_f64(p, *v[f[i]]) for i in range(len(f)))
            worst = max(worst, abs(np.sqrt(float(d)) - d64))
            assert abs(ref.distance_f64(p, *v[f[k]]) - d64) <= BOUND    # the face it names is a nearest one
    print("largest |sqrt(d2) - d64|:", worst)
    assert worst <= BOUND
