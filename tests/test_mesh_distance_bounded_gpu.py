"""mesh_ops.MeshDistance.query(max_distance=...) on the GPU against the numpy definition
(tests/mesh_distance_bounded_reference.py, nearest_within): the same bits of d2 and the same face as the unbounded brute force
for every row within the bound, (inf, -1) beyond it, whatever the grid.  tests/test_mesh_distance_bounded_cpu.py shows that
every bound used here keeps and drops at least a fifth of the points."""
import numpy as np
import pytest
import torch

from tests import mesh_distance_bounded_reference as bref
from tests import mesh_distance_reference as ref
from tests.test_mesh_distance_bounded_cpu import SOUP_D, SOUP_F, lattice_case, soup_case, within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HUGE = 4096.0                                       # a cell this large leaves the whole mesh in one cell


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _md(v, f, **kw):
    from rtg_slam_amd import mesh_ops
    return mesh_ops.MeshDistance(_t(v), _t(f, torch.int32), **kw)


def _equal(got, want, note):
    d2, face = got
    wd, wf = want
    assert d2.dtype == torch.float32 and face.dtype == torch.int32
    assert torch.equal(face.cpu(), torch.from_numpy(wf)), (note, np.nonzero(face.cpu().numpy() != wf)[0][:8])
    assert torch.equal(d2.cpu().view(torch.int32), torch.from_numpy(wd).view(torch.int32)), note


def _same(md, pts, want, max_distance):
    """want: nearest(pts) - the bounded definition follows from it."""
    _equal(md.query(pts, max_distance=max_distance), within(want, bref.max_d2_of(max_distance)), (md.report(), max_distance))


@pytest.mark.parametrize("F", SOUP_F)
def test_soup_every_cell_size(F):
    v, f, pts, want = soup_case(F)
    p = _t(pts)
    cell = _md(v, f).report()["cell"]
    for kw in (dict(), dict(sort=True), dict(cell=0.5 * cell, large_max=8), dict(cell=4 * cell), dict(cell=4 * cell, sort=True), dict(cell=HUGE),
               dict(cell=0.5 * cell, sort=True, large_max=0), dict(cell=0.5 * cell, sort=False, large_max=0)):
        md = _md(v, f, **kw)
        for max_distance in SOUP_D:
            _same(md, p, want, max_distance)
        _equal(md.query(p), want, "unbounded after bounded")


def test_lattice_ties_and_the_boundary():
    v, f, pts, want = lattice_case()
    p = _t(pts)
    below = float(np.nextafter(np.float32(0.125), np.float32(0)))
    for cell in (None, 0.25, 0.125, 0.0625, 0.1, 0.3, 1.0, HUGE):   # ties across cell borders at the first three
        for sort in (False, True):
            md = _md(v, f, cell=cell, sort=sort, large_max=0)
            for max_distance, kept in ((0.125, 1350), (below, 675), (0.5, 2025)):
                _same(md, p, want, max_distance)
                assert int((md.query(p, max_distance=max_distance)[1] >= 0).sum()) == kept


def test_hand_made_faces():
    v, f = ref.hand_made()
    pts = np.concatenate([ref.soup_points(v[:4], f[:4], 1024, 3), v, np.float32([[0.5, 0.5, 0], [0.5, 0.5, 0.25], [0.75, 0.25, 2],
                          [0.25, 0.25, 0], [1, 1, 0.5], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.25, 0.25, 1]])]).astype(np.float32)
    want = ref.nearest(pts, v, f)
    p = _t(pts)
    for max_distance in (0.5, 5.0):
        kept = within(want, bref.max_d2_of(max_distance))[1] >= 0
        assert 0.2 < kept.mean() < 0.8, kept.mean()
        for cell in (None, 0.05, 0.7, HUGE):
            _same(_md(v, f, cell=cell), p, want, max_distance)
            _same(_md(v, f, cell=cell, sort=True), p, want, max_distance)


def test_far_points_and_the_unbounded_limit():
    v, f, _, _ = soup_case(257)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ext = float((hi - lo).max())
    rng = np.random.default_rng(11)
    far = rng.normal(size=(1024, 3))
    far = (100.0 * ext * far / np.linalg.norm(far, axis=1, keepdims=True) + 0.5 * (lo + hi)).astype(np.float32)
    p = _t(far)
    want = ref.nearest(far, v, f)
    for sort in (False, True):
        md = _md(v, f, sort=sort)
        d2, face = md.query(p, max_distance=0.1)
        assert bool((face == -1).all()) and bool(torch.isinf(d2).all()) and bool((d2 > 0).all())
        _equal(md.query(p, max_distance=1e30), want, "max_d2 = inf")       # float32(1e30)^2 = inf: unbounded
        _equal(md.query(p, max_distance=1e30), tuple(x.cpu().numpy() for x in md.query(p)), "against the unbounded kernel")


def test_normals_of_dropped_rows_are_zero():
    v, f, pts, want = soup_case(64)
    md = _md(v, f)
    d2, face, nrm = md.query(_t(pts), normals=True, max_distance=0.25)
    _equal((d2, face), within(want, bref.max_d2_of(0.25)), "with normals")
    dropped = (face < 0).cpu().numpy()
    assert 0.2 < dropped.mean() < 0.8
    got = nrm.cpu().numpy()
    assert not got[dropped].any()
    assert np.array_equal(got.view(np.int32), ref.hit_normals(v, f, face.cpu().numpy()).view(np.int32))
    d2, face, nrm = md.query(_t(pts)[:0], normals=True, max_distance=0.25)
    assert d2.shape == (0,) and face.shape == (0,) and nrm.shape == (0, 3)


def test_bad_bounds_raise():
    v, f = ref.hand_made()
    md = _md(v, f)
    p = _t(np.zeros((4, 3), np.float32))
    for bad in (0, 0.0, -1.0, float("nan"), -float("inf")):
        with pytest.raises(ValueError, match="max_distance"):
            md.query(p, max_distance=bad)
    assert md.report()["queries"] == 0


def test_no_state_survives_a_bounded_call():
    v, f, pts, want = soup_case(257)
    md = _md(v, f)
    p = _t(pts)
    keys = set(md.report())
    a = md.query(p, max_distance=0.05)
    _equal(md.query(p), want, "unbounded after 0.05")
    b = md.query(p, max_distance=0.05)
    _equal(md.query(p, max_distance=4.0), within(want, bref.max_d2_of(4.0)), "4.0 after 0.05")
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    rep = md.report()
    assert set(rep) == keys and rep["queries"] == 4                        # report() keeps exactly its keys
