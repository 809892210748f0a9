"""mesh_ops.register_to_mesh(bounded_query=True) - the per-iteration query under the accumulation's own gate - against
bounded_query=False and the numpy definition (tests/mesh_register_reference.py): the same T to the bit, the same iterations,
inlier counts and reason.  The input is the L-shaped room with 200 outliers 0.5 m off the surface: rows the gate drops, so rows
the bounded query answers with (inf, -1)."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_register_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


@functools.lru_cache(maxsize=None)
def _case():
    src, nrm, v, f, K = ref.room_case()
    assert len(f) == 304 and len(src) == 2000
    pts, mask = ref.room_outliers(src, 200)
    normals = np.empty((len(pts), 3), F32)
    normals[~mask] = nrm
    normals[mask] = (np.float64([0, 0, 1]) @ np.linalg.inv(K)[:3, :3].T).astype(F32)      # the ceiling's, in the source's frame
    return pts, mask, normals, v, f


@functools.lru_cache(maxsize=None)
def _definition(with_normals):
    pts, _, normals, v, f = _case()
    kw = dict(source_normals=normals, min_cos=0.5) if with_normals else {}
    return ref.register(pts, v, f, **kw)


@pytest.mark.parametrize("with_normals", [False, True])
def test_bounded_query_changes_no_bit(with_normals):
    from rtg_slam_amd import mesh_ops
    pts, mask, normals, v, f = _case()
    want_T, want = _definition(with_normals)
    kw = dict(source_normals=_t(normals), min_cos=0.5) if with_normals else {}
    md = mesh_ops.MeshDistance(_t(v), _t(f, torch.int32))
    # the outliers are rows the bound drops: a condition of the input
    d2, face = md.query(_t(pts), max_distance=0.10)
    dropped = (face < 0).cpu().numpy()
    assert dropped[mask].all() and 0 < (~dropped).sum()
    got = {}
    for bounded in (True, False):
        T, rep = mesh_ops.register_to_mesh(_t(pts), md, bounded_query=bounded, **kw)
        got[bounded] = (T, rep)
        print("bounded_query", bounded, {k: rep[k] for k in ("iterations", "inliers", "rank", "reason")})
        assert rep["iterations"] == want["iterations"] and rep["inliers"] == want["inliers"] and rep["reason"] == want["reason"]
        assert rep["rank"] == want["rank"] and rep["converged"] == want["converged"]
        assert np.array_equal(T.view(np.int64), want_T.view(np.int64))
        for k in ("rms_plane_before", "rms_plane_after", "rms_distance_before", "rms_distance_after"):
            assert rep[k] == want[k], k
    (Tb, rb), (Tu, ru) = got[True], got[False]
    assert np.array_equal(Tb, Tu) and set(rb) == set(ru)
    for k in rb:
        if k not in ("query_s", "accumulate_s"):
            assert rb[k] == ru[k], k
    assert max(want["inliers"]) <= 2000                                    # no outlier ever takes part
    T_default, rep_default = mesh_ops.register_to_mesh(_t(pts), md, **kw)  # the default is the bounded query
    assert np.array_equal(T_default, Tb) and rep_default["inliers"] == rb["inliers"]


def test_the_sums_are_the_same_bits():
    """One accumulation over a bounded and an unbounded query of the same moved points: all 30 sums bit for bit."""
    from rtg_slam_amd import mesh_ops
    pts, mask, normals, v, f = _case()
    md = mesh_ops.MeshDistance(_t(v), _t(f, torch.int32))
    p = _t(pts)
    center = ref.box_center(v, f)
    max_d2 = F32(0.10) * F32(0.10)
    d2u, fu = md.query(p)
    d2b, fb = md.query(p, max_distance=0.10)
    assert int((fb < 0).sum()) >= 200 and not torch.equal(fu, fb)
    for sn, min_cos in ((None, 0.0), (_t(normals), 0.5)):
        a = mesh_ops.register_accumulate(p, fu, d2u, md, center, max_d2, sn, min_cos)
        b = mesh_ops.register_accumulate(p, fb, d2b, md, center, max_d2, sn, min_cos)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and a[29] > 0
