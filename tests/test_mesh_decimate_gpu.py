"""The decimation kernels on the MI355X (rtg_slam_amd.mesh_ops.decimate; include/rtgs_slam.h "mesh decimation") against the
numpy definition of tests/mesh_decimate_reference.py, bit for bit (torch.equal on all three arrays, and the stats), on the
generated meshes; on extracted meshes, the invariants; and the layers above with the decimation off."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import mesh_ops, meshing
from tests import mesh_decimate_reference as dr
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


def _against_reference(v, f, c, target, max_error, what):
    want = dr.decimate(v, f, c, target, max_error)
    got = mesh_ops.decimate(*_dev(v, f, c), target, max_error)
    print(what, "target", target, "max_error", max_error, "->", int(got[1].shape[0]), "faces", got[3])
    _assert_equal(got[:3], want[:3], what)
    assert got[3] == want[3], (what, got[3], want[3])
    again = mesh_ops.decimate(*_dev(v, f, c), target, max_error)
    for a, b in zip(got[:3], again[:3]):
        assert torch.equal(a, b)
    assert again[3] == got[3]
    return got


CASES = {"sphere": (lambda: dr.octa_sphere(4), 512, None), "cube": (lambda: dr.cube(10), 300, None),
         "wavy grid": (lambda: dr.grid(33, 0.1), 400, None), "wavy grid, bounded": (lambda: dr.grid(33, 0.1), 0, 0.002),
         "bipyramid": (lambda: dr.bipyramid(200), 100, None), "duplicate vertices": (lambda: dr.grid_with_duplicates(), 300, None)}


@pytest.mark.parametrize("name", list(CASES))
def test_bits_of_the_reference(name):
    make, target, max_error = CASES[name]
    v, f = make()
    got = _against_reference(v, f, dr.colors_for(v, seed=3), target, max_error, name)
    if max_error is None:
        assert got[1].shape[0] == target and got[3]["target_reached"]
    else:
        assert got[1].shape[0] > target and not got[3]["target_reached"]


def test_edge_keys_past_2_31():
    """50 000 unreferenced vertices in front of the sphere: an edge key min V + max passes 2^31; they are gone afterwards."""
    v, f = dr.octa_sphere(4)
    pad = 50000
    v2 = np.concatenate([np.full((pad, 3), 7.0, np.float32), v])
    f2 = f + np.int32(pad)
    assert int(f2.min()) * len(v2) + int(f2.max()) > 2 ** 31
    c2 = dr.colors_for(v2, seed=4)
    got = _against_reference(v2, f2, c2, 512, None, "padded sphere")
    assert got[1].shape[0] == 512 and got[3]["vertices_removed"] == pad + 768
    assert not bool((got[0] == 7.0).all(dim=1).any())                    # (the tie-break hashes the index: not the plain sphere's result)


def test_errors_and_nothing_to_do():
    v, f = dr.cube(10)
    c = dr.colors_for(v, seed=5)
    dv, df, dc = _dev(v, f, c)
    with pytest.raises(ValueError, match="target_faces"):
        mesh_ops.decimate(dv, df, dc, -1)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_error"):
            mesh_ops.decimate(dv, df, dc, 100, bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh_ops.decimate(dv.cpu(), df.cpu(), dc.cpu(), 100)
    with pytest.raises(ValueError, match="face indices"):
        mesh_ops.decimate(dv[:100], df, dc[:100], 100)
    for target in (1200, 5000):
        ov, of, oc, stats = mesh_ops.decimate(dv, df, dc, target)
        assert torch.equal(ov, dv) and torch.equal(of, df) and torch.equal(oc, dc)
        assert stats == {"rounds": 0, "collapses": 0, "faces_removed": 0, "vertices_removed": 0, "target_reached": True}
    none_v, none_f = torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    ov, of, oc, stats = mesh_ops.decimate(none_v, none_f, none_v, 0)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and of.dtype == torch.int32 and stats["rounds"] == 0
    ov, of, oc, stats = mesh_ops.decimate(dv, none_f, dc, 10)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and stats["vertices_removed"] == 602 and stats["target_reached"]


def _shape_facts(faces):
    """What a valid collapse cannot change: the Euler characteristic, the boundary edges, the edges with more than 2 faces,
    whether every directed edge is there once."""
    e = dr.directed_edges(faces)
    V = int(e.max()) + 1
    und, cnt = np.unique(np.minimum(e[:, 0], e[:, 1]) * V + np.maximum(e[:, 0], e[:, 1]), return_counts=True)
    key = e[:, 0] * V + e[:, 1]
    return {"euler": dr.euler(faces), "boundary": int((cnt == 1).sum()), "non_manifold": int((cnt > 2).sum()),
            "oriented": len(np.unique(key)) == len(key)}


def test_extracted_sphere_to_a_quarter():
    tsdf, weight, rgb = tr.sphere_field()
    v, f, c = meshing.TsdfVolume.from_tensors(*_dev(tsdf, weight, rgb), tr.SPHERE_LO, tr.SPHERE_H).extract_mesh()
    F = int(f.shape[0])
    assert F > 10000
    target = F // 4
    ov, of, oc, stats = mesh_ops.decimate(v, f, c, target)
    print("extracted sphere:", int(v.shape[0]), "vertices,", F, "faces ->", int(ov.shape[0]), "vertices,", int(of.shape[0]), "faces", stats)
    assert stats["target_reached"] and target - 1 <= of.shape[0] <= target
    assert stats["faces_removed"] == 2 * stats["collapses"] == F - of.shape[0]
    hf, hof = f.cpu().numpy(), of.cpu().numpy()
    before, after = _shape_facts(hf), _shape_facts(hof)
    print("before", before, "after", after)
    assert before == after and before["euler"] == 2 and before["boundary"] == 0 and before["non_manifold"] == 0 and before["oriented"]
    dr.check_closed_manifold(hof)
    # a subset in order: every output row is an input row, and the rows' input indices ascend
    hv, hov = v.cpu().numpy(), ov.cpu().numpy()
    dr.check_subset_in_order(hov, oc.cpu().numpy(), hv, c.cpu().numpy())
    # on the sphere still: no vertex moved, so the radii are the input's
    r = np.linalg.norm(hov.astype(np.float64) - np.asarray(tr.SPHERE_CENTRE), axis=1)
    r_in = np.linalg.norm(hv.astype(np.float64) - np.asarray(tr.SPHERE_CENTRE), axis=1)
    assert r_in.min() <= r.min() and r.max() <= r_in.max()
    again = mesh_ops.decimate(v, f, c, target)
    for a, b in zip((ov, of, oc), again[:3]):
        assert torch.equal(a, b)
    assert again[3] == stats


def _chain(v, f, c):
    v, f, c, _ = mesh_ops.remove_small_components(v, f, c, 50)
    F = int(f.shape[0])
    v, f, c, stats = mesh_ops.decimate(v, f, c, F // 5)
    return v, f, c, mesh_ops.vertex_normals(v, f), F, stats


def test_box_room_dense_against_sparse_and_chained():
    """One box-room frame at 2 cm: decimated to 20 %, the sparse volume's mesh and the dense one's give the same bits; after
    the removal and before the normals, every vertex that is left has a normal."""
    cam, frames, lo, hi, voxel = tr.box_room_case(1)
    depth, color, pose = frames[0]
    results = []
    for cls in (meshing.TsdfVolume, meshing.SparseTsdfVolume):
        vol = cls(lo, hi, voxel, device=DEV)
        vol.integrate(depth.to(DEV), color.to(DEV), cam, pose)
        results.append(_chain(*vol.extract_mesh()))
    dense, sparse = results
    for a, b in zip(dense[:4], sparse[:4]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    v, f, c, n, F, stats = dense
    print("box-room frame:", F, "faces ->", int(f.shape[0]), stats)
    assert F > 10000 and stats == sparse[5]
    assert stats["target_reached"] and F // 5 - 1 <= f.shape[0] <= F // 5
    assert n.shape == v.shape and not bool(torch.isnan(n).any())
    assert int((n.abs().sum(dim=1) == 0).sum()) == 0                     # every vertex is referenced after the compaction
    assert torch.equal(torch.unique(f.reshape(-1).long()), torch.arange(v.shape[0], device=DEV))


def test_layers_above_with_the_decimation_off():
    cam, frames, lo, hi, voxel = tr.box_room_case(1)
    stream = [(d.to(DEV), col.to(DEV), p) for d, col, p in frames]
    call = lambda **kw: meshing.mesh_from_map(None, cam, None, iter(stream), voxel=voxel, depth_source="sensor", bounds=(lo, hi), device=DEV, **kw)
    for options in ({}, {"min_component_faces": 50, "simplify_cell": 3 * voxel, "normals": True}):
        plain, off = call(**options), call(decimate=0.0, **options)
        assert len(plain) == len(off)
        assert list(plain[3]) == list(off[3])                            # the same keys in the same order
        for a, b in zip(plain[:3] + plain[4:], off[:3] + off[4:]):
            assert a.dtype == b.dtype and torch.equal(a, b)
    v, f, c = plain[:3]
    a = mesh_ops.clean_mesh(v, f, c, min_component_faces=20, normals=True)
    b = mesh_ops.clean_mesh(v, f, c, min_component_faces=20, normals=True, decimate_faces=0, decimate_max_error=None)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert a[4] == b[4] and list(a[4]) == list(b[4])
    # and on: the new keys beside the removal's, the report's new keys, the face count
    F = int(a[1].shape[0])
    on = mesh_ops.clean_mesh(v, f, c, min_component_faces=20, normals=True, decimate_faces=F // 2)
    assert set(on[4]) == set(a[4]) | {"decimate_rounds", "decimate_collapses", "decimate_faces_removed", "decimate_vertices_removed",
                                      "decimate_target_reached"}
    assert {k: on[4][k] for k in a[4]} == a[4] and F // 2 - 1 <= on[1].shape[0] <= F // 2 and on[3].shape == on[0].shape
    res = call(decimate=0.25, decimate_max_error=0.05, normals=True)
    rep = res[3]
    assert set(rep) - set(plain[3]) == {"decimate", "decimate_max_error", "F_before_decimate", "decimate_rounds", "decimate_collapses",
                                        "decimate_target_reached", "decimate_s"}
    assert rep["F_before_decimate"] == rep["F_raw"] and rep["F"] == res[1].shape[0] and rep["V"] == res[0].shape[0] == res[4].shape[0]
    if rep["decimate_target_reached"]:
        assert int(0.25 * rep["F_raw"]) - 1 <= rep["F"] <= int(0.25 * rep["F_raw"])
    for bad in ({"decimate": 1.0}, {"decimate": -0.1}, {"decimate_max_error": 0.01}, {"decimate": 0.5, "decimate_max_error": 0.0}):
        with pytest.raises(ValueError, match="decimate"):
            call(**bad)
