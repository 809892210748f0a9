"""The mesh clean-up kernels on the MI355X (rtg_slam_amd.mesh_ops; include/rtgs_slam.h "mesh operations") against the numpy
definition of tests/mesh_ops_reference.py, bit for bit (torch.equal throughout): vertex normals, component labels,
small-component removal, compaction and vertex clustering, on hand-made meshes and on extracted ones."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import mesh_ops, meshing
from tests import mesh_ops_reference as mr
from tests import tsdf_reference as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _assert_equal(got, want, what=""):
    """A tuple of device tensors against the reference's arrays: same dtype, same shape, same bits."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        w = torch.from_numpy(np.ascontiguousarray(w))
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g, w), (what, i, int((g != w).sum()))


def _sphere_volume(extra=None):
    tsdf, weight, rgb = tr.sphere_field()
    if extra is not None:
        tsdf = np.minimum(tsdf, extra)
    return meshing.TsdfVolume.from_tensors(*_dev(tsdf, weight, rgb), tr.SPHERE_LO, tr.SPHERE_H)


@pytest.fixture(scope="module")
def sphere():
    """The sphere of tsdf_reference.sphere_field() extracted on the device, and the same arrays on the host; read-only."""
    v, f, c = _sphere_volume().extract_mesh()
    assert v.shape[0] > 5000 and f.shape[0] > 10000
    return (v, f, c), (v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy())


# ---- normals ---------------------------------------------------------------------------------------------------------

def test_normals_fan_longer_than_a_wave():
    v, f = mr.fan(200, seed=1)
    assert np.bincount(f.reshape(-1)).max() == 200                       # one vertex has 200 corners: more than 64
    want = mr.vertex_normals(v, f)
    got = mesh_ops.vertex_normals(*_dev(v, f))
    _assert_equal((got,), (want,), "fan")
    assert torch.equal(got, mesh_ops.vertex_normals(*_dev(v, f)))


def test_normals_degenerate_mesh():
    v, f = mr.degenerate_mesh()
    got = mesh_ops.vertex_normals(*_dev(v, f))
    _assert_equal((got,), (mr.vertex_normals(v, f),), "degenerate")
    assert torch.equal(got[5:].cpu(), torch.zeros(2, 3)) and not torch.isnan(got).any()
    # no faces at all, and no vertices at all
    assert torch.equal(mesh_ops.vertex_normals(_dev(v)[0], torch.zeros(0, 3, dtype=torch.int32, device=DEV)).cpu(), torch.zeros(7, 3))
    assert mesh_ops.vertex_normals(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV)).shape == (0, 3)


def test_normals_sphere(sphere):
    (v, f, _), (hv, hf, _) = sphere
    got = mesh_ops.vertex_normals(v, f)
    _assert_equal((got,), (mr.vertex_normals(hv, hf),), "sphere")
    n = got.cpu().numpy().astype(np.float64)
    radial = hv.astype(np.float64) - np.asarray(tr.SPHERE_CENTRE)
    nonzero = np.abs(n).sum(axis=1) > 0
    assert nonzero.mean() > 0.99
    dots = np.einsum("ij,ij->i", n[nonzero], radial[nonzero] / np.linalg.norm(radial[nonzero], axis=1, keepdims=True))
    print("normal . radial: min", dots.min(), "mean", dots.mean())
    assert (dots > 0).all()                                              # wound towards free space: outwards
    assert np.abs(np.linalg.norm(n[nonzero], axis=1) - 1).max() < 1e-6


# ---- labels ----------------------------------------------------------------------------------------------------------

def test_labels_strip_with_permuted_indices():
    f, V = mr.strip(5000, seed=2)
    got = mesh_ops.component_labels(_dev(f)[0], V)
    _assert_equal((got,), (mr.component_labels(f, V),), "strip")
    assert bool((got == 0).all())                                        # one component: its smallest index is 0
    assert torch.equal(got, mesh_ops.component_labels(_dev(f)[0], V))


def test_labels_random_small_components():
    f, V = mr.random_components(300, seed=4)
    want = mr.component_labels(f, V)
    assert len(np.unique(want)) == 300 + 7                               # and 7 vertices nobody references
    got = mesh_ops.component_labels(_dev(f)[0], V)
    _assert_equal((got,), (want,), "components")


def test_labels_isolated_vertices():
    none = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    assert torch.equal(mesh_ops.component_labels(none, 1000).cpu(), torch.arange(1000, dtype=torch.int32))
    assert mesh_ops.component_labels(none, 0).shape == (0,)
    f = np.array([[900, 17, 500]], dtype=np.int32)
    want = np.arange(1000, dtype=np.int32)
    want[[900, 500]] = 17
    _assert_equal((mesh_ops.component_labels(_dev(f)[0], 1000),), (want,), "one face")
    with pytest.raises(ValueError, match="face indices"):
        mesh_ops.component_labels(_dev(f)[0], 900)


# ---- removal ---------------------------------------------------------------------------------------------------------

def test_removal_restores_the_sphere(sphere):
    """The sphere plus a blob of 3 voxels radius 11 voxels off its surface, the two fields combined by min: removing the
    small component gives back the extraction of the sphere alone, in all three arrays (order is preserved)."""
    (v, f, c), (hv, hf, hc) = sphere
    nx, ny, nz = tr.SPHERE_DIMS
    x = tr.axis_centres(tr.SPHERE_LO[0], nx, tr.SPHERE_H).astype(np.float64)[None, None, :]
    y = tr.axis_centres(tr.SPHERE_LO[1], ny, tr.SPHERE_H).astype(np.float64)[None, :, None]
    z = tr.axis_centres(tr.SPHERE_LO[2], nz, tr.SPHERE_H).astype(np.float64)[:, None, None]
    d = np.sqrt((x - 0.62) ** 2 + (y - 0.61) ** 2 + (z - 0.63) ** 2) - 3 * tr.SPHERE_H
    blob = np.clip(d / (4 * tr.SPHERE_H), -1.0, 1.0).astype(np.float32)
    bv, bf, bc = _sphere_volume(blob).extract_mesh()
    n_blob = int(bf.shape[0]) - int(f.shape[0])
    print("sphere faces", int(f.shape[0]), "blob faces", n_blob)
    assert 20 < n_blob < int(f.shape[0]) // 4 and bv.shape[0] > v.shape[0]
    rv, rf, rc, stats = mesh_ops.remove_small_components(bv, bf, bc, n_blob + 1)
    assert torch.equal(rv, v) and torch.equal(rf, f) and torch.equal(rc, c)
    assert stats == {"components": 2, "components_removed": 1, "faces_removed": n_blob,
                     "vertices_removed": int(bv.shape[0]) - int(v.shape[0])}
    # exactly min_faces stays
    kv, kf, kc, stats = mesh_ops.remove_small_components(bv, bf, bc, n_blob)
    assert torch.equal(kv, bv) and torch.equal(kf, bf) and torch.equal(kc, bc) and stats["components_removed"] == 0
    # against the reference, and everything removed
    want = mr.remove_small_components(bv.cpu().numpy(), bf.cpu().numpy(), bc.cpu().numpy(), n_blob + 1)
    _assert_equal((rv, rf, rc), want[:3], "removal")
    assert want[3] == {"components": 2, "components_removed": 1, "faces_removed": n_blob,
                       "vertices_removed": int(bv.shape[0]) - int(v.shape[0])}
    ev, ef, ec, stats = mesh_ops.remove_small_components(bv, bf, bc, int(bf.shape[0]))
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and ec.shape == (0, 3) and stats["components_removed"] == 2


def test_removal_and_compact_on_random_components():
    f, V = mr.random_components(300, seed=6)
    rng = np.random.default_rng(7)
    v = rng.standard_normal((V, 3)).astype(np.float32)
    c = mr.colors_for(v, seed=8)
    for min_faces in (0, 1, 6, 7, 13):
        got = mesh_ops.remove_small_components(*_dev(v, f, c), min_faces)
        want = mr.remove_small_components(v, f, c, min_faces)
        _assert_equal(got[:3], want[:3], f"min_faces {min_faces}")
        assert got[3] == want[3], (min_faces, got[3], want[3])
    _assert_equal(mesh_ops.compact(*_dev(v, f, c)), mr.compact(v, f, c), "compact")


# ---- clustering ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("voxels", [2.0, 3.5])
def test_clustering_sphere(sphere, voxels):
    (v, f, c), (hv, hf, hc) = sphere
    cell = voxels * tr.SPHERE_H
    got = mesh_ops.simplify_clusters(v, f, c, cell, tr.SPHERE_LO)
    want = mr.simplify_clusters(hv, hf, hc, cell, tr.SPHERE_LO)
    _assert_equal(got, want, f"cell {cell}")
    keys = mr.cluster_keys(mr.cluster_cells(hv, cell, tr.SPHERE_LO))
    assert got[0].shape[0] == len(np.unique(keys)) and 0 < got[1].shape[0] < f.shape[0]
    print("cell", cell, "V", int(v.shape[0]), "->", int(got[0].shape[0]), "F", int(f.shape[0]), "->", int(got[1].shape[0]))
    # every output vertex lies in its own cell
    assert np.array_equal(mr.cluster_keys(mr.cluster_cells(got[0].cpu().numpy(), cell, tr.SPHERE_LO)), np.unique(keys))


def test_clustering_cells_with_more_than_256_members():
    rng = np.random.default_rng(9)
    v = rng.uniform(0.0, 1.0, (3000, 3)).astype(np.float32)
    f = rng.integers(0, len(v), (5000, 3)).astype(np.int32)
    f[100:140] = f[60:100]                                               # identical faces ...
    f[140:180] = f[60:100][:, [1, 2, 0]]                                 # ... rotated ones ...
    f[180:220] = f[60:100][:, [0, 2, 1]]                                 # ... and mirrored ones
    c = mr.colors_for(v, seed=10)
    counts = np.bincount(mr.cluster_keys(mr.cluster_cells(v, 0.5, (0.0, 0.0, 0.0))))
    assert len(counts) == 8 and counts.min() > 256
    _assert_equal(mesh_ops.simplify_clusters(*_dev(v, f, c), 0.5, (0.0, 0.0, 0.0)),
                  mr.simplify_clusters(v, f, c, 0.5, (0.0, 0.0, 0.0)), "big cells")
    # a finer grid keeps most faces, so the duplicate rule decides something
    got = mesh_ops.simplify_clusters(*_dev(v, f, c), 0.07, (0.0, 0.0, 0.0))
    want = mr.simplify_clusters(v, f, c, 0.07, (0.0, 0.0, 0.0))
    _assert_equal(got, want, "fine cells")
    assert 4000 < want[1].shape[0] < 5000 - 70


def test_clustering_origin_below_world_zero():
    v, f = mr.fan(50, seed=11)
    v = v - np.float32(2.0)                                              # every coordinate negative
    c = mr.colors_for(v, seed=12)
    assert (v < 0).all()
    origin = (-3.75, -3.6, -3.5)
    _assert_equal(mesh_ops.simplify_clusters(*_dev(v, f, c), 0.3, origin), mr.simplify_clusters(v, f, c, 0.3, origin), "origin")
    with pytest.raises(ValueError, match="below origin"):
        mesh_ops.simplify_clusters(*_dev(v, f, c), 0.3, (-3.75, -2.0, -3.5))
    # all vertices in one cell: one vertex, no faces
    ov, of, oc = mesh_ops.simplify_clusters(*_dev(v, f, c), 10.0, origin)
    assert ov.shape == (1, 3) and of.shape == (0, 3) and of.dtype == torch.int32


# ---- chaining --------------------------------------------------------------------------------------------------------

def _chain(v, f, c, min_faces, cell, origin):
    v, f, c, stats = mesh_ops.remove_small_components(v, f, c, min_faces)
    v, f, c = mesh_ops.simplify_clusters(v, f, c, cell, origin)
    return v, f, c, mesh_ops.vertex_normals(v, f)


def test_chain_twice_and_sparse_against_dense():
    """One box-room frame at 2 cm: the sparse volume's mesh equals the dense one's, and removal, clustering and normals
    chained on either give the same bits, run after run, and the reference's."""
    cam, frames, lo, hi, voxel = tr.box_room_case(1)
    depth, color, pose = frames[0]
    meshes = []
    for cls in (meshing.TsdfVolume, meshing.SparseTsdfVolume):
        vol = cls(lo, hi, voxel, device=DEV)
        vol.integrate(depth.to(DEV), color.to(DEV), cam, pose)
        meshes.append((vol.extract_mesh(), vol.lo))
    (dense, dlo), (sparse, slo) = meshes
    assert dense[1].shape[0] > 10000
    a = _chain(*dense, 50, 3 * voxel, dlo)
    b = _chain(*dense, 50, 3 * voxel, dlo)
    s = _chain(*sparse, 50, 3 * voxel, slo)
    for x, y, z in zip(a, b, s):
        assert torch.equal(x, y) and torch.equal(x, z)
    hv, hf, hc = (t.cpu().numpy() for t in dense)
    rv, rf, rc, _ = mr.remove_small_components(hv, hf, hc, 50)
    rv, rf, rc = mr.simplify_clusters(rv, rf, rc, 3 * voxel, dlo)
    _assert_equal(a, (rv, rf, rc, mr.vertex_normals(rv, rf)), "chain")
    print("box-room frame:", hv.shape[0], "vertices,", hf.shape[0], "faces ->", rv.shape[0], "vertices,", rf.shape[0], "faces")
    # each operation by itself, twice
    for op in (lambda: (mesh_ops.vertex_normals(dense[0], dense[1]),), lambda: (mesh_ops.component_labels(dense[1], dense[0].shape[0]),),
               lambda: mesh_ops.remove_small_components(*dense, 50)[:3], lambda: mesh_ops.simplify_clusters(*dense, 2.5 * voxel, dlo)):
        for x, y in zip(op(), op()):
            assert torch.equal(x, y)
