"""rtgs_mesh_register_accumulate and mesh_ops.register_to_mesh on the GPU against the numpy definition
(tests/mesh_register_reference.py): the same bits of the 30 sums, the same iterations and inlier counts, the same T."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_distance_reference as mdr
from tests import mesh_register_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
MAX_D2 = F32(0.1) * F32(0.1)
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 5, 70_000]


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def _md(v, f, **kw):
    from rtg_slam_amd import mesh_ops
    return mesh_ops.MeshDistance(_t(v), _t(f, torch.int32), **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _soup():
    """About 200 faces, two of them degenerate, a pool of 3 * 1024 + 5 points near them with their brute-force (d2, face), and
    unit source normals: mostly the hit face's, tilted."""
    v, f = mdr.soup(200, seed=31, box=1.0)
    f = f.copy()
    f[17] = [f[17, 0], f[17, 0], f[17, 1]]                          # two equal corners
    f[140] = [f[140, 2], f[140, 2], f[140, 2]]                      # three
    n = 3 * 1024 + 5
    p, _ = ref.sample(v, np.delete(f, [17, 140], axis=0), n, 32)
    rng = np.random.default_rng(33)
    pts = (p + rng.normal(0, 0.03, p.shape)).astype(F32)
    d2, face = mdr.nearest(pts, v, f)
    sn = mdr.face_unit_normals(v, f)[face].astype(np.float64) + rng.normal(0, 0.6, (n, 3))
    sn = (sn / np.linalg.norm(sn, axis=1, keepdims=True)).astype(F32)
    return v, f, pts, d2, face, sn


@functools.lru_cache(maxsize=None)
def _rows(N):
    """N rows drawn from the pool, with the rows every gate needs written over them."""
    v, f, pts, d2, face, sn = _soup()
    rng = np.random.default_rng(100 + N)
    pick = rng.integers(0, len(pts), N) if N > len(pts) else rng.permutation(len(pts))[:N]
    p, d, k, s = pts[pick].copy(), d2[pick].copy(), face[pick].copy(), sn[pick].copy()
    if N >= 63:
        k[3], k[N - 1] = -1, -1                                      # no face
        d[5], d[N - 2] = MAX_D2, MAX_D2                              # exactly at the gate: kept
        d[7] = np.nextafter(MAX_D2, F32(1))                          # just over it: dropped
        d[9], d[10] = np.inf, np.nan
        k[11], d[11] = 17, F32(1e-4)                                 # dropped by the normal gate only
        k[12], d[12] = 140, F32(1e-4)
        k[13] = 20                                                   # a sound face
        nh = mdr.face_unit_normals(v, f)[k[13]]
        s[13] = np.cross(nh, [1, 0, 0] if abs(nh[0]) < 0.9 else [0, 1, 0]).astype(F32)   # across the hit normal: source gate only
        s[13] /= np.linalg.norm(s[13])
        d[13] = F32(1e-4)
    return p, d, k, s


@pytest.mark.parametrize("N", SIZES)
def test_accumulate_equals_the_definition(N):
    from rtg_slam_amd import mesh_ops
    v, f = _soup()[:2]
    p, d, k, s = _rows(N)
    md = _md(v, f)
    center = ref.box_center(v, f)
    tp, td, tk, ts = _t(p.reshape(-1, 3)), _t(d), _t(k, torch.int32), _t(s.reshape(-1, 3))
    for normals, min_cos in ((None, 0.0), (s, 0.5)):
        want = ref.accumulate(p, k, d, v, f, center, MAX_D2, normals, min_cos)
        got = mesh_ops.register_accumulate(tp, tk, td, md, center, MAX_D2, None if normals is None else ts, min_cos)
        again = mesh_ops.register_accumulate(tp, tk, td, md, center, MAX_D2, None if normals is None else ts, min_cos)
        assert got.dtype == torch.float64 and got.shape == (30,)
        print(N, "count", want[29], "sum r^2", want[27])
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (N, got.cpu().numpy() - want)
        assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    if N >= 63:
        kept = ref.takes_part(k, d, mdr.face_unit_normals(v, f)[np.maximum(k, 0)], MAX_D2)
        assert kept[5] and kept[N - 2] and not kept[[3, N - 1, 7, 9, 10, 11, 12]].any() and kept[13]
        dot = np.abs((s * mdr.face_unit_normals(v, f)[np.maximum(k, 0)]).sum(1))
        assert dot[13] < 1e-6 and 0 < (kept & (dot < 0.5)).sum() < kept.sum()      # the source gate decides for some rows
    if N == 0:
        assert not got.cpu().numpy().any()


def _cases():
    src, nrm, v, f, _ = ref.room_case()
    pts, _ = ref.room_outliers(src, len(src) // 10)
    ws, wv, wf = ref.wall_case()
    return {"room": (src, v, f, {}), "room_normals": (src, v, f, dict(source_normals=nrm, min_cos=0.5)),
            "outliers": (pts, v, f, {}), "wall": (ws, wv, wf, {})}


@pytest.mark.parametrize("name", ["room", "room_normals", "outliers", "wall"])
def test_register_equals_the_definition(name):
    from rtg_slam_amd import mesh_ops
    pts, v, f, kw = _cases()[name]
    want_T, want = ref.register(pts, v, f, **kw)
    dkw = {k: (_t(x) if k == "source_normals" else x) for k, x in kw.items()}
    results = []
    for sort in (True, False):
        T, rep = mesh_ops.register_to_mesh(_t(pts), _md(v, f, sort=sort), **dkw)
        results.append(T)
        print(name, "sort", sort, {k: rep[k] for k in ("iterations", "inliers", "rank", "reason", "rotation_deg", "translation_m")},
              "largest |T - T_definition|", np.abs(T - want_T).max())
        assert T.dtype == np.float64 and T.shape == (4, 4)
        assert rep["iterations"] == want["iterations"] and rep["inliers"] == want["inliers"]
        assert rep["rank"] == want["rank"] and rep["converged"] == want["converged"] and rep["reason"] == want["reason"]
        # every device step is held to bits and the host arithmetic is the same float64 numpy: the same T to the bit
        assert np.array_equal(_bits(T), _bits(want_T))
        for k in ("rms_plane_before", "rms_plane_after", "rms_distance_before", "rms_distance_after"):
            assert rep[k] == want[k], k
        assert rep["inlier_share"] == want["inliers"][-1] / len(pts) and rep["query_s"] > 0 and rep["accumulate_s"] > 0
    assert np.array_equal(results[0], results[1])                    # the target's sort setting changes the time only
    if name == "wall":
        assert rep["rank"] == 3
    if name == "room":
        from tests.test_mesh_register_cpu import BOUND, displacement
        assert displacement(T, ref.KNOWN, pts) <= BOUND
        assert abs(rep["rotation_deg"] - 1.5) < 1e-3 and 0 < rep["translation_m"] < 0.07


def test_too_few_inliers_and_init():
    from rtg_slam_amd import mesh_ops
    src, _, v, f, K = ref.room_case()
    md = _md(v, f)
    T, rep = mesh_ops.register_to_mesh(_t(src[:5]), md)
    assert rep["reason"] == "too few inliers" and not rep["converged"] and rep["iterations"] == 0 and rep["inliers"] == [5]
    assert np.array_equal(T, np.eye(4))
    far = (src[:50] + F32(5)).astype(F32)
    T, rep = mesh_ops.register_to_mesh(_t(far), md, init=K)
    assert rep["reason"] == "too few inliers" and rep["inliers"] == [0] and np.array_equal(T, K) and rep["inlier_share"] == 0
    T, rep = mesh_ops.register_to_mesh(_t(src[:0]), md)
    assert rep["reason"] == "too few inliers" and rep["inliers"] == [0]
    want_T, want = ref.register(src, v, f, max_iterations=2)
    T, rep = mesh_ops.register_to_mesh(_t(src), md, max_iterations=2)
    assert rep["reason"] == "max iterations" and not rep["converged"] and rep["iterations"] == 2 and np.array_equal(T, want_T)


def test_bad_input_raises():
    from rtg_slam_amd import mesh_ops
    src, nrm, v, f, _ = ref.room_case()
    md = _md(v, f)
    p = _t(src)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh_ops.register_to_mesh(torch.from_numpy(src), md)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh_ops.register_to_mesh(p, md, source_normals=torch.from_numpy(nrm))
    with pytest.raises(ValueError, match=r"\[N,3\] float32"):
        mesh_ops.register_to_mesh(p.double(), md)
    with pytest.raises(ValueError, match=r"\[N,3\] float32"):
        mesh_ops.register_to_mesh(p[:, :2], md)
    with pytest.raises(ValueError, match="source_normals"):
        mesh_ops.register_to_mesh(p, md, source_normals=_t(nrm[:-1]))
    with pytest.raises(ValueError, match="max_distance"):
        mesh_ops.register_to_mesh(p, md, max_distance=0.0)
    with pytest.raises(ValueError, match="max_iterations"):
        mesh_ops.register_to_mesh(p, md, max_iterations=0)
    with pytest.raises(ValueError, match="init"):
        mesh_ops.register_to_mesh(p, md, init=np.eye(3))
    with pytest.raises(ValueError, match="MeshDistance"):
        mesh_ops.register_to_mesh(p, (v, f))
    d2, face = md.query(p)
    with pytest.raises(ValueError, match="face must be"):
        mesh_ops.register_accumulate(p, face[:-1], d2, md, (0, 0, 0), 0.01)
    with pytest.raises(RuntimeError, match="HIP device"):
        mesh_ops.register_accumulate(p, face.cpu(), d2, md, (0, 0, 0), 0.01)


def test_align_to_gt():
    from rtg_slam_amd import evaluation, mesh_ops
    from tests.test_mesh_register_cpu import BOUND, displacement
    src, nrm, v, f, K = ref.room_case()
    # the source in a frame of its own: transform brings it to the room's, up to KNOWN
    pose = ref.rigid((0.1, 0.9, -0.2), 25.0, (0.3, -0.2, 0.1))
    local = ref.apply(np.linalg.inv(pose), src).astype(F32)
    local_n = (nrm.astype(np.float64) @ pose[:3, :3]).astype(F32)
    reports = {}
    T_total, rep = evaluation.align_to_gt(_t(local), v, f, transform=pose, source_normals=_t(local_n), min_cos=0.5, reports=reports)
    T_align = T_total @ np.linalg.inv(pose)
    err = displacement(T_align, K, src)
    print("align_to_gt: residual displacement", err, rep["inliers"])
    # local and the product pose @ local are rounded to float32 once more than the CPU case's source: 2^-24 of 1.5 m, twice
    assert err <= BOUND + 2 * 1.5 * 2.0 ** -24 and rep["converged"] and reports["gt"]["queries"] == len(rep["inliers"])
    # more points than sample_nums: the draw of eval_pcd's subsample, shared with the normals
    gen = torch.Generator().manual_seed(3)
    T2, rep2 = evaluation.align_to_gt(_t(local), _t(v), _t(f, torch.int32), transform=pose, sample_nums=500, generator=gen)
    pick = torch.randperm(len(local), generator=torch.Generator().manual_seed(3))[:500].numpy()
    from rtg_slam_amd import slam_ops as so
    moved = so.transform_map(_t(local[pick]), torch.from_numpy(pose.astype(F32)))
    want, _ = mesh_ops.register_to_mesh(moved, _md(v, f))
    assert np.array_equal(T2, want @ pose) and rep2["inliers"][0] <= 500
