"""The definition of the bounded point-to-mesh query (tests/mesh_distance_bounded_reference.py) and the inputs the GPU tests
hold the kernel to: that every bound they use both keeps and drops a good share of the points - a test of the bound whose bound
never bites tests nothing."""
import functools

import numpy as np
import pytest

from tests import mesh_distance_bounded_reference as bref
from tests import mesh_distance_reference as ref

F32 = np.float32
SOUP_F = (1, 64, 257, 2000)
SOUP_D = (0.05, 0.25, 1.0, 4.0)
SOUP_N = 512


@functools.lru_cache(maxsize=None)
def soup_case(F):
    """-> (vertices, faces, points, nearest(points)): shared with tests/test_mesh_distance_bounded_gpu.py, never modified."""
    v, f = ref.soup(F, seed=F)
    pts = ref.soup_points(v, f, SOUP_N, seed=F + 1)
    return v, f, pts, ref.nearest(pts, v, f)


@functools.lru_cache(maxsize=None)
def lattice_case():
    v, f = ref.lattice()
    pts = ref.lattice_points()
    return v, f, pts, ref.nearest(pts, v, f)


def within(want, max_d2):
    """nearest_within from a nearest() result computed once."""
    d2, face = want
    keep = (d2 <= F32(max_d2)) & (face >= 0)
    return np.where(keep, d2, F32(np.inf)).astype(F32), np.where(keep, face, -1).astype(np.int32)


def test_max_d2_of():
    assert bref.max_d2_of(0.125) == F32(0.015625) and bref.max_d2_of(0.125).dtype == F32
    assert bref.max_d2_of(0.1) == F32(0.1) * F32(0.1)                      # register_to_mesh's md * md
    assert np.isinf(bref.max_d2_of(1e30)) and bref.max_d2_of(0.0) == 0


def test_lattice_boundary_is_kept_by_equality():
    v, f, pts, want = lattice_case()
    assert len(pts) == 2700
    values, counts = np.unique(want[0], return_counts=True)
    assert values.tolist() == [0.0, 0.015625, 0.25, 4.0] and counts.tolist() == [675] * 4
    below = np.nextafter(F32(0.125), F32(0))
    for max_distance, kept in ((0.125, 1350), (below, 675), (0.5, 2025)):
        max_d2 = bref.max_d2_of(max_distance)
        d2, face = bref.nearest_within(pts, v, f, max_d2)
        keep = face >= 0
        assert int(keep.sum()) == kept, (max_distance, int(keep.sum()))
        assert np.array_equal(d2[keep], want[0][keep]) and np.array_equal(face[keep], want[1][keep])
        assert np.isinf(d2[~keep]).all() and (want[0][~keep] > max_d2).all()
        assert all(np.array_equal(a, b) for a, b in zip((d2, face), within(want, max_d2)))
    assert bref.max_d2_of(0.125) == F32(0.015625) and bref.max_d2_of(below) < F32(0.015625)


@pytest.mark.parametrize("F", SOUP_F)
def test_every_soup_bound_keeps_and_drops(F):
    v, f, pts, want = soup_case(F)
    for max_distance in SOUP_D:
        max_d2 = bref.max_d2_of(max_distance)
        d2, face = bref.nearest_within(pts, v, f, max_d2)
        keep = face >= 0
        share = keep.mean()
        print(F, max_distance, "kept", share)
        assert 0.2 <= share <= 0.8, (F, max_distance, share)               # a condition of the input
        assert np.array_equal(keep, want[0] <= max_d2)
        assert np.array_equal(d2[keep].view(np.int32), want[0][keep].view(np.int32)) and np.array_equal(face[keep], want[1][keep])
        assert np.isinf(d2[~keep]).all() and d2.dtype == F32 and face.dtype == np.int32
        assert all(np.array_equal(a, b) for a, b in zip((d2, face), within(want, max_d2)))


def test_edge_values():
    v, f = ref.hand_made()
    pts = np.concatenate([ref.soup_points(v[:4], f[:4], 256, 3), v, F32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]])]).astype(F32)
    want = ref.nearest(pts, v, f)
    d2, face = bref.nearest_within(pts, v, f, F32(np.inf))                 # unbounded
    assert np.array_equal(d2.view(np.int32), want[0].view(np.int32)) and np.array_equal(face, want[1])
    assert face[-3:].tolist() == [-1, -1, -1] and np.isinf(d2[-3:]).all()  # the non-finite points, whatever the bound
    d2, face = bref.nearest_within(pts, v, f, F32(0))                      # only exact zeros
    zero = want[0] == 0
    assert zero.sum() >= len(v) - 1 and not zero.all()                     # every corner a face uses lies on it
    assert np.array_equal(face >= 0, zero) and (d2[zero] == 0).all() and np.isinf(d2[~zero]).all()
    assert np.array_equal(face[zero], want[1][zero])
    d2, face = bref.nearest_within(pts[-3:], v, f, bref.max_d2_of(5.0))
    assert face.tolist() == [-1, -1, -1] and np.isinf(d2).all()


def test_truncated_composition_keeps_the_fractions():
    """eval_mesh_surface_truncated against eval_mesh_surface on a pair where some samples lie beyond the bound."""
    gv, gf = ref.lattice(4, 0.25)
    rv = gv.copy()
    rv[rv[:, 0] == 0.5, 2] = 0.2                                           # a lifted strip
    rng = np.random.default_rng(0)

    def draw(v, f, n):
        fi = rng.integers(0, len(f), n)
        uv = rng.random((n, 2))
        flip = uv.sum(1) > 1
        uv[flip] = 1 - uv[flip]
        a, b, c = (v[f[fi, j]].astype(np.float64) for j in range(3))
        return (a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a)).astype(F32), fi.astype(np.int32)

    rp, ro = draw(rv, gf, 400)
    gp, go = draw(gv, gf, 400)
    full = ref.eval_mesh_surface(rp, ro, rv, gf, gp, go, gv, gf, (0.03,))
    cut = bref.eval_mesh_surface_truncated(rp, ro, rv, gf, gp, go, gv, gf, (0.03,), 0.05)
    assert set(cut) == set(full) | {"max_distance", "beyond_acc", "beyond_comp"}
    for k in ("P (< 0.03)", "R (< 0.03)", "F1 (< 0.03)"):
        assert cut[k] == full[k], k
    assert 0 < cut["beyond_acc"] < 400 and 0 < cut["beyond_comp"] < 400
    assert cut["accuracy"] < full["accuracy"] and cut["completion"] < full["completion"]
    assert cut["normal_samples_acc"] == 400 - cut["beyond_acc"] and cut["normal_samples_comp"] == 400 - cut["beyond_comp"]
