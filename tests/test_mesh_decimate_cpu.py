"""The decimation rule itself (tests/mesh_decimate_reference.py, the numpy definition the kernels of csrc/mesh_decimate.hip are
held to): what it guarantees on closed, open, flat, sharp and high-valence meshes, and its quality against the vertex
clustering that exists.  No GPU."""
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import mesh_decimate_reference as dr
from tests import mesh_ops_reference as mr


@pytest.fixture(scope="module")
def meshes():
    """name -> (vertices, faces, colors); read-only."""
    out = {}
    for name, (v, f) in (("sphere", dr.octa_sphere(4)), ("cube", dr.cube(10)), ("flat", dr.grid(33, 0.0)),
                         ("wavy", dr.grid(33, 0.1)), ("bipyramid", dr.bipyramid(200))):
        out[name] = (v, f, dr.colors_for(v, seed=len(out)))
    return out


def _volume(v, f):
    """The signed volume in exact rational arithmetic (a float32 is a rational number)."""
    total = Fraction(0)
    for tri in f.tolist():
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = ([Fraction(float(x)) for x in v[i]] for i in tri)
        total += ax * (by * cz - bz * cy) - ay * (bx * cz - bz * cx) + az * (bx * cy - by * cx)
    return total / 6


def test_generators(meshes):
    assert [meshes[k][0].shape[0] for k in ("sphere", "cube", "flat", "bipyramid")] == [1026, 602, 1089, 202]
    assert [meshes[k][1].shape[0] for k in ("sphere", "cube", "flat", "bipyramid")] == [2048, 1200, 2048, 400]
    for k in ("sphere", "cube", "bipyramid"):
        dr.check_closed_manifold(meshes[k][1])
        assert dr.euler(meshes[k][1]) == 2 and _volume(*meshes[k][:2]) > 0          # wound outwards
    assert _volume(*meshes["cube"][:2]) == 1
    dr.check_open_manifold(meshes["flat"][1])
    assert dr.euler(meshes["flat"][1]) == 1 and len(dr.boundary_edges(meshes["flat"][1])) == 128
    assert np.sort(np.bincount(meshes["bipyramid"][1].reshape(-1)))[-2:].tolist() == [200, 200]


@pytest.mark.parametrize("target", [1024, 512, 200])
def test_sphere_stays_a_closed_manifold(meshes, target):
    v, f, c = meshes["sphere"]
    ov, of, oc, stats = dr.decimate(v, f, c, target)
    assert of.shape == (target, 3) and of.dtype == np.int32 and ov.dtype == np.float32 and oc.dtype == np.float32
    dr.check_closed_manifold(of)
    assert dr.euler(of) == 2
    assert len(np.unique(of)) == len(ov) and of.max() == len(ov) - 1
    dr.check_subset_in_order(ov, oc, v, c)
    assert stats == {"rounds": stats["rounds"], "collapses": (2048 - target) // 2, "faces_removed": 2048 - target,
                     "vertices_removed": (2048 - target) // 2, "target_reached": True}
    print("sphere to", target, stats)


@pytest.mark.parametrize("max_error", [None, 1e-5])
def test_cube_keeps_its_shape_exactly(meshes, max_error):
    v, f, c = meshes["cube"]
    ov, of, oc, stats = dr.decimate(v, f, c, 300, max_error)
    assert of.shape == (300, 3) and stats["target_reached"]
    dr.check_closed_manifold(of)
    assert dr.euler(of) == 2
    assert _volume(ov, of) == 1
    centroid = ov.astype(np.float64)[of].mean(axis=1)
    err = np.abs(np.abs(centroid).max(axis=1) - 0.5).max()
    print("cube to 300, max_error", max_error, stats, "centroid error", err)
    assert err == 0.0
    dr.check_subset_in_order(ov, oc, v, c)


def test_cube_error_bound_stops_above_the_target(meshes):
    v, f, c = meshes["cube"]
    ov, of, oc, stats = dr.decimate(v, f, c, 12, 1e-5)
    print("cube to 12 with max_error 1e-5 stops at", len(of), stats)
    assert len(of) > 12 and stats["target_reached"] is False and stats["rounds"] < dr.MAX_ROUNDS
    dr.check_closed_manifold(of)
    assert _volume(ov, of) == 1


def test_flat_grid_keeps_its_boundary(meshes):
    v, f, c = meshes["flat"]
    ov, of, oc, stats = dr.decimate(v, f, c, 200)
    assert of.shape == (200, 3) and stats["target_reached"]
    dr.check_open_manifold(of)
    assert dr.euler(of) == 1
    # the boundary edges as pairs of positions: no boundary vertex was removed, no boundary edge changed
    as_points = lambda vv, ff: sorted(tuple(sorted((tuple(vv[a].tolist()), tuple(vv[b].tolist())))) for a, b in dr.boundary_edges(ff))
    assert as_points(ov, of) == as_points(v, f)


def test_wavy_grid_stops_by_itself_under_an_error_bound(meshes):
    v, f, c = meshes["wavy"]
    ov, of, oc, stats = dr.decimate(v, f, c, 0, 0.002)
    print("wavy grid, max_error 0.002, target 0 stops at", len(of), stats)
    assert 0 < len(of) < 2048 and stats["target_reached"] is False and stats["rounds"] < dr.MAX_ROUNDS
    dr.check_open_manifold(of)
    assert dr.euler(of) == 1 and len(dr.boundary_edges(of)) == 128


@pytest.mark.parametrize("target", [100, 0])
def test_bipyramid_apexes_survive(meshes, target):
    v, f, c = meshes["bipyramid"]
    ov, of, oc, stats = dr.decimate(v, f, c, target)
    print("bipyramid to", target, len(of), stats)
    dr.check_closed_manifold(of)
    assert dr.euler(of) == 2 and len(of) <= max(target, 6)
    for apex in (200, 201):
        assert (ov == v[apex]).all(axis=1).any()


def test_duplicate_vertices_are_welded():
    """Vertices that share a position (surface extraction leaves them where the field is exactly zero at a grid point) span
    area-less faces and can leave a vertex without a normal.  A collapse between two of them changes no face, so it passes
    the flip test and, costing next to nothing, comes first: the area-less faces go, and every vertex left has a normal."""
    v, f = dr.grid_with_duplicates()
    c = dr.colors_for(v, seed=9)
    area = lambda vv, ff: np.linalg.norm(np.cross(vv.astype(np.float64)[ff[:, 1]] - vv.astype(np.float64)[ff[:, 0]],
                                                  vv.astype(np.float64)[ff[:, 2]] - vv.astype(np.float64)[ff[:, 0]]), axis=1)
    no_normal = lambda vv, ff: int((np.abs(mr.vertex_normals(vv, ff)).sum(axis=1) == 0).sum())
    assert int((area(v, f) == 0).sum()) == 16 and no_normal(v, f) == 1
    for target in (400, 100):
        ov, of, oc, stats = dr.decimate(v, f, c, target)
        assert len(of) == target and stats["target_reached"]
        assert int((area(ov, of) == 0).sum()) == 0 and no_normal(ov, of) == 0
        dr.check_open_manifold(of)
        assert dr.euler(of) == 1 and len(dr.boundary_edges(of)) == 64


def test_errors_and_nothing_to_do(meshes):
    v, f, c = meshes["cube"]
    with pytest.raises(ValueError):
        dr.decimate(v, f, c, -1)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            dr.decimate(v, f, c, 100, bad)
    for target in (1200, 5000):
        ov, of, oc, stats = dr.decimate(v, f, c, target)
        assert np.array_equal(ov, v) and np.array_equal(of, f) and np.array_equal(oc, c)
        assert stats == {"rounds": 0, "collapses": 0, "faces_removed": 0, "vertices_removed": 0, "target_reached": True}
    # unreferenced vertices go even then; empty meshes work
    v2 = np.concatenate([np.zeros((3, 3), np.float32), v])
    ov, of, oc, stats = dr.decimate(v2, f + 3, np.concatenate([np.ones((3, 3), np.float32), c]), 1200)
    assert np.array_equal(ov, v) and np.array_equal(of, f) and np.array_equal(oc, c) and stats["vertices_removed"] == 3
    none = np.zeros((0, 3), np.float32)
    ov, of, oc, stats = dr.decimate(none, np.zeros((0, 3), np.int32), none, 0)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and of.dtype == np.int32 and stats["rounds"] == 0 and stats["target_reached"]
    ov, of, oc, stats = dr.decimate(v, np.zeros((0, 3), np.int32), c, 10)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and stats["vertices_removed"] == len(v)


def test_the_hash_breaks_the_sweep(meshes, monkeypatch):
    """Ranking equal costs by the vertex index alone makes the independent set a sweep: many more rounds on a regular mesh."""
    v, f, c = meshes["cube"]
    with_hash = dr.decimate(v, f, c, 300)[3]["rounds"]
    monkeypatch.setattr(dr, "vertex_hash", lambda u: np.zeros(len(u), np.int64))
    without = dr.decimate(v, f, c, 300)[3]["rounds"]
    print("cube to 300: rounds with the hash", with_hash, "without", without)
    assert with_hash < without


@pytest.mark.parametrize("cell", [0.25, 0.4])
def test_quality_against_vertex_clustering(meshes, cell):
    """At the face count clustering produces, the decimated sphere's faces lie closer to the sphere than the clustered ones."""
    v, f, c = meshes["sphere"]
    cv, cf, cc = mr.simplify_clusters(v, f, c, cell, (-1.01, -1.01, -1.01))
    ov, of, oc, stats = dr.decimate(v, f, c, len(cf))
    assert stats["target_reached"] and len(cf) - 1 <= len(of) <= len(cf)
    off = lambda vv, ff: float(np.abs(np.linalg.norm(vv.astype(np.float64)[ff].mean(axis=1), axis=1) - 1).mean())
    print("cell", cell, "faces", len(cf), "mean | |centroid| - 1 |: decimated", off(ov, of), "clustered", off(cv, cf))
    assert off(ov, of) <= off(cv, cf)


def test_options_of_the_layers_above():
    from rtg_slam_amd import __main__ as cli, mesh_ops, meshing
    p = cli.build_parser()
    opts = p.parse_args(["mesh", "--config", "x.yaml"])
    assert opts.decimate == 0.0 and opts.decimate_max_error is None
    opts = p.parse_args(["mesh", "--config", "x.yaml", "--decimate", "0.25", "--decimate-max-error", "0.01"])
    assert opts.decimate == 0.25 and opts.decimate_max_error == 0.01
    for bad in ({"decimate": 1.0}, {"decimate": -0.5}, {"decimate": float("nan")}, {"decimate_max_error": 0.01},
                {"decimate": 0.5, "decimate_max_error": -1.0}):
        with pytest.raises(ValueError, match="decimate"):
            meshing.mesh_from_map(None, None, [np.eye(4)], None, bounds=((0, 0, 0), (1, 1, 1)), **bad)
    import torch
    none = torch.zeros(0, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh_ops.decimate(none, torch.zeros(0, 3, dtype=torch.int32), none, 0)
    assert (mesh_ops.DECIMATE_MIN_VALENCE, mesh_ops.DECIMATE_MAX_VALENCE, mesh_ops.DECIMATE_MAX_ROUNDS) == \
        (dr.MIN_VALENCE, dr.MAX_VALENCE, dr.MAX_ROUNDS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtgs_slam.h")).read()
    for name, value in (("MIN_VALENCE", dr.MIN_VALENCE), ("MAX_VALENCE", dr.MAX_VALENCE), ("MAX_ROUNDS", dr.MAX_ROUNDS)):
        assert f"#define RTGS_MESH_DECIMATE_{name} {value}\n" in header
