"""The definition of the mesh registration (tests/mesh_register_reference.py) against known answers.  No GPU."""
import functools
import math

import numpy as np

from tests import mesh_distance_reference as mdr
from tests import mesh_register_reference as ref

F32 = np.float32

# The bound on the residual displacement max_i |T p_i - KNOWN p_i| over the source points of room_case(): the samples are rounded
# to float32 (2^-24 of coordinates up to 1.3 m: 8e-8 m), every iteration moves them by float32(T), and the loop stops after an
# update below 1e-6, so no bound follows from the stopping rule alone.  As tests/test_mesh_distance_cpu.py does, the largest
# value over this file's cases was measured with this definition - MEASURED - and the bound is 4 x that, which covers another
# numpy or BLAS build.
MEASURED = 3.74e-8                                                 # metres: room_case() without normals
BOUND = 4 * MEASURED


def displacement(T, K, pts):
    return float(np.linalg.norm(ref.apply(T, pts) - ref.apply(K, pts), axis=1).max())


@functools.lru_cache(maxsize=None)
def room_run():
    src, nrm, v, f, K = ref.room_case()
    return src, nrm, v, f, K, ref.register(src, v, f)


def test_the_room_is_what_the_cases_need():
    v, f = ref.room()
    assert 250 < len(f) < 350 and f.min() == 0 and f.max() == len(v) - 1
    assert np.linalg.norm(v.astype(np.float64) - ref.box_center(v, f), axis=1).max() <= 1.5
    n = mdr.face_unit_normals(v, f)
    assert (np.abs(n).max(axis=1) == 1).all()                       # axis-aligned, none degenerate
    # closed: every edge has exactly two faces
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    assert (counts == 2).all()
    src, _, _, _, K = ref.room_case()
    moved = np.linalg.norm(ref.apply(K, src) - src.astype(np.float64), axis=1).max()
    assert np.isclose(np.linalg.norm(K[:3, 3]), 0.027) and moved <= 0.066


def test_recovers_the_known_transform():
    src, nrm, v, f, K, (T, rep) = room_run()
    err = displacement(T, K, src)
    print("iterations", rep["iterations"], "inliers", rep["inliers"], "residual displacement", err)
    assert rep["inliers"][0] == len(src) == 2000
    assert rep["converged"] and rep["reason"] == "converged" and rep["rank"] == 6 and rep["iterations"] < 10
    assert err <= BOUND
    assert rep["rms_plane_before"] > 0.01 and rep["rms_plane_after"] < 1e-6 and rep["rms_distance_after"] < 1e-6
    # with the samples' own normals and min_cos = 0.5 some samples near an edge start on a perpendicular face and sit out
    T2, rep2 = ref.register(src, v, f, source_normals=nrm, min_cos=0.5)
    err2 = displacement(T2, K, src)
    print("with normals: inliers", rep2["inliers"], "residual displacement", err2)
    assert rep2["inliers"][0] < len(src) and rep2["inliers"][-1] == len(src) and rep2["converged"] and err2 <= BOUND
    # from an init that already holds the answer: one small update
    T3, rep3 = ref.register(src, v, f, init=T)
    assert rep3["iterations"] == 1 and rep3["converged"] and displacement(T3, K, src) <= BOUND


def test_a_wall_constrains_three_degrees_of_freedom():
    src, v, f = ref.wall_case()
    T, rep = ref.register(src, v, f)
    assert rep["rank"] == 3 and rep["converged"] and rep["inliers"][0] == len(src)
    n = mdr.face_unit_normals(v, f)[0].astype(np.float64)
    c = ref.box_center(v, f).astype(np.float64)
    # the first solve: the twist has no component along the dropped eigenvectors
    moved = ref.transform_f32(src, np.eye(4))
    d2, face = mdr.nearest(moved, v, f)
    out = ref.accumulate(moved, face, d2, v, f, c, F32(0.1) * F32(0.1))
    x, rank, lam, E = ref.solve(out)
    assert rank == 3 and (lam[:3] <= 1e-8 * lam[5]).all() and np.array_equal(x, rep["twists"][0])
    for j in range(3):
        assert abs(np.dot(E[:, j], x)) <= 1e-12 * np.linalg.norm(x), j
    # what it leaves alone: no rotation about the normal, no translation in the plane - up to the 2^-23 by which the float32
    # normals of the wall's eight faces differ from face 0's
    assert abs(np.dot(x[:3], n)) <= 1e-6 * np.linalg.norm(x[:3])
    assert np.linalg.norm(x[3:] - np.dot(x[3:], n) * n) <= 1e-6 * np.linalg.norm(x[3:])
    # and what it finds: the centre comes back by the 1 cm offset, the tilt is undone
    back = ref.apply(T, c[None])[0] - c
    print("wall: centre moved by", back, "plane rms after", rep["rms_plane_after"])
    assert abs(np.dot(back, n) + 0.01) < 1e-6
    angle = np.degrees(np.arccos(np.clip(0.5 * (np.trace(T[:3, :3]) - 1), -1, 1)))
    assert abs(angle - 0.5) < 1e-3


def test_outliers_stay_outside_the_gate():
    src, _, v, f, K, (T, rep) = room_run()
    pts, mask = ref.room_outliers(src, len(src) // 10)
    assert mask.sum() == 200 and len(pts) == 2200
    T2, rep2 = ref.register(pts, v, f)
    assert rep2["inliers"] == rep["inliers"] == [len(src)] * len(rep["inliers"])
    # exactly those: at the start and at the end the outliers, and only they, are beyond the gate
    for M in (np.eye(4), T2):
        d2, _ = mdr.nearest(ref.transform_f32(pts, M), v, f)
        assert np.array_equal(d2 > F32(0.1) * F32(0.1), mask)
    err = displacement(T2, K, src)
    print("with outliers: residual displacement", err, "largest |T - T_clean|", np.abs(T2 - T).max())
    assert err <= BOUND and displacement(T2, T, src) <= BOUND


def test_too_few_inliers():
    src, _, v, f, _, _ = room_run()
    T, rep = ref.register(src[:5], v, f)
    assert rep["reason"] == "too few inliers" and not rep["converged"] and rep["iterations"] == 0 and np.array_equal(T, np.eye(4))
    far = (src[:50] + F32(5)).astype(F32)
    T, rep = ref.register(far, v, f, init=ref.KNOWN)
    assert rep["reason"] == "too few inliers" and rep["inliers"] == [0] and np.array_equal(T, ref.KNOWN)
    assert np.isnan(rep["rms_plane_before"])


def test_hand_made_accumulations():
    v = F32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    f = np.int32([[0, 1, 2], [0, 2, 3]])                             # z = 0 with n = (0, 0, 1); x = 0 with n = (1, 0, 0)
    center = F32([0.5, 0.25, 0])
    want = np.zeros(30)
    # p = (0.25, 0.5, 2) above face 0: q = (-0.25, 0.25, 2), r = 2, J = (q.y, -q.x, 0, 0, 0, 1) = (0.25, 0.25, 0, 0, 0, 1)
    J, r = np.array([0.25, 0.25, 0, 0, 0, 1.0]), 2.0
    k = 0
    for i in range(6):
        for j in range(i, 6):
            want[k] = J[i] * J[j]
            k += 1
    want[21:27], want[27], want[28], want[29] = J * r, 4.0, 4.0, 1.0
    one = ref.accumulate(F32([[0.25, 0.5, 2]]), [0], F32([4]), v, f, center, F32(4))
    assert np.array_equal(one, want) and one[0] == 0.0625 and one[5] == 0.25 and one[20] == 1 and one[26] == 2
    # p = (-0.5, 0.25, 0.25) beside face 1: q = (-1, 0, 0.25), r = -0.5, J = (0, q.z, -q.y, 1, 0, 0) = (0, 0.25, 0, 1, 0, 0)
    J2, r2 = np.array([0, 0.25, 0, 1.0, 0, 0]), -0.5
    want2 = np.zeros(30)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            want2[k] = J2[i] * J2[j]
            k += 1
    want2[21:27], want2[27], want2[28], want2[29] = J2 * r2, 0.25, 0.25, 1.0
    two = ref.accumulate(F32([[0.25, 0.5, 2], [-0.5, 0.25, 0.25]]), [0, 1], F32([4, 0.25]), v, f, center, F32(4))
    assert np.array_equal(two, want + want2)
    # the gates: face -1, d2 over max_d2 (equality keeps), a source normal across the face's
    pts = F32([[0.25, 0.5, 2]] * 4)
    sn = F32([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 0.8, 0.6]])
    got = ref.accumulate(pts, [0, 0, 0, 0], F32([4, 4, 4, 4]), v, f, center, F32(4), sn, 0.6)
    assert np.array_equal(got, 3 * want)                              # |n . s| = 1, 1, 0, 0.6
    got = ref.accumulate(pts, [0, -1, 0, 0], F32([4, 4, np.nextafter(F32(4), F32(5)), np.inf]), v, f, center, F32(4))
    assert np.array_equal(got, want)
    assert np.array_equal(ref.accumulate(pts[:0], [], F32([]), v, f, center, F32(4)), np.zeros(30))


def test_the_order_of_summation():
    rng = np.random.default_rng(5)
    for N in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 5, 300 * 1024 + 7):
        t = rng.normal(size=(N, 2)) * 10.0 ** rng.integers(-8, 8, (N, 1))
        got = ref.ordered_sum(t)
        exact = np.array([math.fsum(t[:, k]) for k in range(2)])
        assert (np.abs(got - exact) <= N * 2.0 ** -52 * np.abs(t).sum(0)).all(), N
    # integers sum exactly whatever the order, and the order is the documented one for a case small enough to write out
    t = np.arange(1, 2 * 1024 + 4, dtype=np.float64)[:, None]
    assert ref.ordered_sum(t)[0] == t.sum()
    t = np.zeros((1024 + 2, 1))
    t[[0, 256, 1, 64, 1024, 1025], 0] = [1e16, 1.0, 1.0, -1e16, 1.0, 3.0]
    # chunk 0: slot 0 = 1e16 + 1 = 1e16, slot 1 = 1, wave 0 = (1e16 + 1 (slot 1, at the last step)) = 1e16, wave 1 = -1e16:
    # chunk 0 = 0; chunk 1 = 1 + 3 = 4
    assert ref.ordered_sum(t)[0] == 4.0
