"""The numpy definition of the mesh clean-up (tests/mesh_ops_reference.py) against hand-made cases, and the PLY writer's
normals.  No GPU: the kernels are held to this definition in tests/test_mesh_ops_gpu.py."""
import numpy as np
import pytest

from rtg_slam_amd import io_formats as iof
from tests import mesh_ops_reference as mr

F32 = np.float32


def test_tetrahedron_normals_point_outwards():
    v, f = mr.tetrahedron()
    n = mr.vertex_normals(v, f)
    assert n.dtype == F32 and n.shape == (4, 3)
    # by symmetry a corner's normal is its own direction from the centroid
    want = v / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(n - want).max() < 1e-6
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
    # the face normals themselves: e1 x e2 of the first face, by hand
    fn = mr.face_normals(v, f)
    assert np.array_equal(fn[0], np.cross(v[1] - v[0], v[2] - v[0]).astype(F32))
    assert (np.einsum("ij,ij->i", fn, v[f].mean(axis=1)) > 0).all()


def test_normals_of_unreferenced_and_arealess_vertices_are_zero():
    v, f = mr.degenerate_mesh()
    n = mr.vertex_normals(v, f)
    assert np.array_equal(n[6], np.zeros(3, F32))                       # referenced by nobody
    assert np.array_equal(n[5], np.zeros(3, F32))                       # only an area-less face
    assert np.array_equal(n[0], np.array([0, 0, 1], F32))
    assert np.isfinite(n).all()


def test_two_triangles_sharing_a_vertex_are_one_component():
    f = np.array([[4, 1, 2], [2, 3, 5]], dtype=np.int32)
    lab = mr.component_labels(f, 7)
    assert lab.dtype == np.int32
    assert lab.tolist() == [0, 1, 1, 1, 1, 1, 6]                        # 0 and 6 are unreferenced: they label themselves
    g = np.array([[4, 1, 2], [0, 3, 5]], dtype=np.int32)
    assert mr.component_labels(g, 6).tolist() == [0, 1, 1, 0, 1, 0]


def test_labels_do_not_depend_on_the_order_of_the_faces():
    f, V = mr.random_components(40, seed=3)
    a = mr.component_labels(f, V)
    b = mr.component_labels(f[::-1], V)
    assert np.array_equal(a, b)
    assert (a <= np.arange(V)).all()
    assert np.array_equal(a[a], a)


def _two_fans(k_small, k_big=9):
    """A fan of k_big faces on vertices 0.., then one of k_small, then an unreferenced vertex."""
    faces = [(0, j + 1, j + 2) for j in range(k_big)]
    b = k_big + 2
    faces += [(b, b + j + 1, b + j + 2) for j in range(k_small)]
    V = b + k_small + 2 + 1
    v = np.arange(3 * V, dtype=F32).reshape(V, 3)
    return v, np.asarray(faces, dtype=np.int32), mr.colors_for(v)


def test_component_of_exactly_min_faces_is_kept_and_one_less_is_dropped():
    v, f, c = _two_fans(5)
    ov, of, oc, stats = mr.remove_small_components(v, f, c, 5)           # sizes 9 and 5: both stay, the loose vertex goes
    assert np.array_equal(of, f) and np.array_equal(ov, v[:-1]) and np.array_equal(oc, c[:-1])
    assert stats == {"components": 2, "components_removed": 0, "faces_removed": 0, "vertices_removed": 1}
    v, f, c = _two_fans(4)
    ov, of, oc, stats = mr.remove_small_components(v, f, c, 5)           # sizes 9 and 4 = min_faces - 1
    assert np.array_equal(of, f[:9]) and np.array_equal(ov, v[:11]) and np.array_equal(oc, c[:11])
    assert stats == {"components": 2, "components_removed": 1, "faces_removed": 4, "vertices_removed": 7}


def test_removal_keeps_order_and_reindexes():
    v, f, c = _two_fans(3)
    f = np.concatenate([f[9:], f[:9]])                                   # the small component first
    v, c = v[::-1].copy(), c[::-1].copy()
    f = (len(v) - 1 - f).astype(np.int32)
    ov, of, oc, _ = mr.remove_small_components(v, f, c, 4)
    assert len(of) == 9 and len(ov) == 11
    assert np.array_equal(ov[of], v[f[3:]]) and np.array_equal(oc[of], c[f[3:]])
    assert np.array_equal(ov, v[-11:])                                   # the survivors in their order
    cv, cf, cc = mr.compact(ov, of, oc)
    assert np.array_equal(cv, ov) and np.array_equal(cf, of) and np.array_equal(cc, oc)


def test_cluster_boundary_vertex_goes_to_the_upper_cell():
    origin, cell = (-1.0, -1.0, -1.0), 0.5
    v = np.array([[-0.5, -1.0, -0.75], [np.nextafter(F32(-0.5), F32(-1)), -0.5, 0.0]], dtype=F32)
    assert mr.cluster_cells(v, cell, origin).tolist() == [[1, 0, 0], [0, 1, 2]]
    with pytest.raises(ValueError, match="below origin"):
        mr.cluster_cells(np.array([[-1.0, -1.0001, 0.0]], F32), cell, origin)


def test_cluster_all_vertices_in_one_cell_gives_no_faces():
    v, f = mr.tetrahedron()
    c = mr.colors_for(v)
    vs = v * F32(0.1)
    ov, of, oc = mr.simplify_clusters(vs, f, c, 1.0, (-0.5, -0.5, -0.5))
    assert ov.shape == (1, 3) and of.shape == (0, 3) and of.dtype == np.int32
    assert np.array_equal(ov[0], (vs.astype(np.float64).sum(0) / 4.0).astype(F32))
    assert np.array_equal(oc[0], (c.astype(np.float64).sum(0) / 4.0).astype(F32))


def test_cluster_duplicate_face_rule():
    # unit cells from origin 0; vertices 0..3 sit in cells A < B < C < D (keys ascend with x), 4..6 repeat A, B, C
    v = np.array([[0.5, 0, 0], [1.5, 0, 0], [2.5, 0, 0], [3.5, 0, 0], [0.25, 0, 0], [1.25, 0, 0], [2.25, 0, 0]], dtype=F32)
    f = np.array([[1, 2, 0],      # (A, B, C) after rotation
                  [4, 5, 6],      # the same face: dropped
                  [0, 2, 1],      # mirrored (A, C, B): another face, stays
                  [0, 4, 3],      # two corners in A: dropped
                  [6, 3, 5],      # (B, C, D) after rotation
                  [2, 4, 5]],     # (A, B, C) again, rotated: dropped
                 dtype=np.int32)
    ov, of, oc = mr.simplify_clusters(v, f, mr.colors_for(v), 1.0, (0.0, 0.0, 0.0))
    assert ov.shape == (4, 3)
    assert of.tolist() == [[0, 1, 2], [0, 2, 1], [1, 2, 3]]
    assert np.array_equal(ov[:, 0], np.array([0.375, 1.375, 2.375, 3.5], F32))


def test_cluster_every_output_vertex_lies_in_its_own_cell():
    rng = np.random.default_rng(5)
    v = rng.uniform(-1.0, 1.0, (4000, 3)).astype(F32)
    f = rng.integers(0, len(v), (6000, 3)).astype(np.int32)
    origin, cell = (-1.0, -1.0, -1.0), 0.13
    ov, of, oc = mr.simplify_clusters(v, f, mr.colors_for(v), cell, origin)
    cells_in = mr.cluster_cells(v, cell, origin)
    nc = cells_in.max(axis=0) + 1
    want = np.unique((cells_in[:, 2] * nc[1] + cells_in[:, 1]) * nc[0] + cells_in[:, 0])
    cells_out = mr.cluster_cells(ov, cell, origin)
    got = (cells_out[:, 2] * nc[1] + cells_out[:, 1]) * nc[0] + cells_out[:, 0]
    # exact: the mean of values in [a, b) rounds into [a, b] and rounding, subtraction, division and floor are monotone -
    # the recomputed key of an output vertex is the key of its cell
    assert np.array_equal(got, want)
    assert len(of) > 0 and of.min() >= 0 and of.max() < len(ov)
    assert (of[:, 0] < of[:, 1]).all() and (of[:, 0] < of[:, 2]).all() and (of[:, 1] != of[:, 2]).all()
    assert len(np.unique(of, axis=0)) == len(of)


def _expected_ply(v, f, c=None, n=None):
    """The documented layout, built by hand: header, then per vertex x y z [nx ny nz] [r g b], then per face 3 i j k."""
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + [f"property float {a}" for a in "xyz"]
    if n is not None:
        head += [f"property float {a}" for a in ("nx", "ny", "nz")]
    if c is not None:
        head += [f"property uchar {a}" for a in ("red", "green", "blue")]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    body = b""
    q = None if c is None else np.clip(np.rint(c.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    for i in range(len(v)):
        body += v[i].astype("<f4").tobytes()
        if n is not None:
            body += n[i].astype("<f4").tobytes()
        if q is not None:
            body += q[i].tobytes()
    for tri in f:
        body += b"\x03" + tri.astype("<i4").tobytes()
    return ("\n".join(head) + "\n").encode("ascii") + body


def test_save_mesh_ply_with_normals_round_trips_and_without_is_unchanged(tmp_path):
    v, f = mr.fan(12, seed=2)
    c = mr.colors_for(v, seed=4)
    n = mr.vertex_normals(v, f)
    for colors in (None, c):
        plain, with_n = str(tmp_path / "plain.ply"), str(tmp_path / "normals.ply")
        iof.save_mesh_ply(plain, v, f, colors)
        assert open(plain, "rb").read() == _expected_ply(v, f, colors)          # byte for byte what the writer wrote before
        iof.save_mesh_ply(with_n, v, f, colors, normals=n)
        assert open(with_n, "rb").read() == _expected_ply(v, f, colors, n)
        lv, lf, lc = iof.load_mesh_ply(with_n, with_colors=True)
        assert np.array_equal(lv.astype(F32), v) and lv.dtype == np.float64      # bit-equal: float32 -> float64 is exact
        assert np.array_equal(lf, f.astype(np.int64))
        if colors is None:
            assert lc is None
        else:
            assert np.array_equal(np.rint(lc * 255), np.rint(c.astype(np.float64) * 255))
    with pytest.raises(ValueError, match="normals"):
        iof.save_mesh_ply(str(tmp_path / "bad.ply"), v, f, c, normals=n[:-1])


def test_mesh_ops_refuse_cpu_tensors():
    import torch
    from rtg_slam_amd import mesh_ops
    v, f = mr.tetrahedron()
    tv, tf, tc = torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(mr.colors_for(v))
    for call in (lambda: mesh_ops.vertex_normals(tv, tf), lambda: mesh_ops.component_labels(tf, 4),
                 lambda: mesh_ops.compact(tv, tf, tc), lambda: mesh_ops.remove_small_components(tv, tf, tc, 2),
                 lambda: mesh_ops.simplify_clusters(tv, tf, tc, 0.5, (-2, -2, -2))):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
