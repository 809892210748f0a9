"""evaluation.eval_mesh_surface(max_distance=D) on the GPU against the numpy composition
(tests/mesh_distance_bounded_reference.py, eval_mesh_surface_truncated): a distance beyond D counts as D, the fractions below
the threshold are exactly those of the call without the bound."""
import functools

import numpy as np
import pytest

from tests import mesh_distance_bounded_reference as bref
from tests import mesh_distance_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, THRES, D = 20_000, (0.03,), 0.05


@functools.lru_cache(maxsize=None)
def _meshes():
    """The GT lattice (4 m x 4 m in z = 0) and the reconstruction: the same lattice with a strip of vertices lifted by 0.2 m."""
    gv, gf = ref.lattice()
    rv = gv.copy()
    rv[(gv[:, 0] >= 1.0) & (gv[:, 0] <= 1.5), 2] = 0.2
    return rv, gf.copy(), gv, gf


@functools.lru_cache(maxsize=None)
def _want():
    from rtg_slam_amd import io_formats as iof
    rv, rf, gv, gf = _meshes()
    rp, ro = iof.sample_mesh_surface(rv, rf, N, 0)
    gp, go = iof.sample_mesh_surface(gv, gf, N, 0)
    return bref.eval_mesh_surface_truncated(rp.astype(np.float32), ro, rv, rf, gp.astype(np.float32), go, gv, gf, THRES, D)


def test_truncated_equals_the_composition():
    from rtg_slam_amd import evaluation
    rv, rf, gv, gf = _meshes()
    want = _want()
    assert 0 < want["beyond_acc"] < N and 0 < want["beyond_comp"] < N       # the lifted strip: a condition of the input
    reports = {}
    got = evaluation.eval_mesh_surface(rv, rf, gv, gf, dist_thres=THRES, sample_nums=N, seed=0, device=DEV, reports=reports, max_distance=D)
    full = evaluation.eval_mesh_surface(rv, rf, gv, gf, dist_thres=THRES, sample_nums=N, seed=0, device=DEV)
    assert set(got) == set(want) == set(full) | {"max_distance", "beyond_acc", "beyond_comp"}
    assert list(got)[:len(full)] == list(full)                             # the keys it had, in their order, then the three
    assert set(reports) == {"gt", "rec"} and reports["gt"]["queries"] == 1
    for k, w in want.items():
        print(k, got[k], w, full.get(k))
        if k.startswith(("P ", "R ", "F1 ", "normal_samples", "beyond", "max_distance")):
            assert got[k] == w, k                                          # counts: exact
        else:
            # float64 sums of N positive terms in two different orders: they differ by at most N 2^-53 of the sum
            assert abs(got[k] - w) <= 1e-12 * abs(w), k
    for k in ("P (< 0.03)", "R (< 0.03)", "F1 (< 0.03)"):
        assert got[k] == full[k], k
    assert 0 < got["P (< 0.03)"] < 100 and got["accuracy"] < full["accuracy"] and got["completion"] < full["completion"]
    assert got["normal_samples_acc"] == N - got["beyond_acc"] and got["normal_samples_comp"] == N - got["beyond_comp"]
    assert full["normal_samples_acc"] == N


def test_the_bound_must_exceed_the_threshold():
    from rtg_slam_amd import evaluation
    rv, rf, gv, gf = _meshes()
    for bad in (0.03, 0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_distance"):
            evaluation.eval_mesh_surface(rv, rf, gv, gf, dist_thres=THRES, sample_nums=100, device=DEV, max_distance=bad)
