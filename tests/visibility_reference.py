"""Plain-numpy float32 restatement of the visibility cull (include/rtgs_slam.h, "visibility"; evaluation.VisibilityCull):
which points a depth frame saw, which faces that leaves, and the culled mesh.  Used only by tests; it is the definition the
kernels of csrc/visibility.hip are held to, bit for bit.  Also the grid meshes (the flat box room and the cube annex behind
its wall) the CPU and the command-line tests share."""
import numpy as np

from tests import mesh_ops_reference as mr
from tests.tsdf_reference import w2c_from_c2w

F32 = np.float32


def views_add(views, points, depth, K, c2w, tolerance):
    """One frame into views [N] int32, in place.  points [N,3] float32 in the frame c2w maps into; depth [H,W] float32 metres;
    K = (fx, fy, cx, cy).  The chain of tsdf_reference.integrate on a given point; returns the number of points seen."""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    depth = np.ascontiguousarray(depth, dtype=F32)
    assert views.dtype == np.int32 and views.shape == (len(p),)
    H, W = depth.shape
    fx, fy, cx, cy = (F32(k) for k in K)
    tolerance = F32(tolerance)
    M = w2c_from_c2w(c2w)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        xc = ((M[0, 0] * x + M[0, 1] * y) + M[0, 2] * z) + M[0, 3]
        yc = ((M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z) + M[1, 3]
        zc = ((M[2, 0] * x + M[2, 1] * y) + M[2, 2] * z) + M[2, 3]
        assert xc.dtype == F32 and zc.dtype == F32
        ok = zc > 0
        u = fx * xc / zc + cx
        v = fy * yc / zc + cy
        pu = np.floor(u + F32(0.5))
        pv = np.floor(v + F32(0.5))
        assert pu.dtype == F32
        ok &= (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
        idx = np.nonzero(ok)[0]
        d = depth[pv[idx].astype(np.int64), pu[idx].astype(np.int64)]
        keep = d > 0
        idx, d = idx[keep], d[keep]
        behind = (zc[idx] - d) > tolerance
        assert (zc[idx] - d).dtype == F32
    idx = idx[~behind]
    views[idx] += 1
    return int(idx.size)


def keep_faces(faces, views, min_views, any_vertex):
    """-> int32 [F]: 1 where all three corners (any_vertex: at least one) have views >= min_views."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    seen = np.asarray(views)[f] >= min_views
    return (seen.any(axis=1) if any_vertex else seen.all(axis=1)).astype(np.int32)


def cull_mesh(vertices, faces, views, min_views, any_vertex):
    """-> (vertices, faces): the kept faces in their order, the vertices they use in theirs, faces re-indexed - the compaction
    of mesh_ops_reference under a keep mask."""
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    ov, of, _ = mr._compact(v, f, v, keep_faces(f, views, min_views, any_vertex).astype(bool))
    return ov, of


# ---------------------------------------------------------------------------------------------------------------------
# grid meshes
# ---------------------------------------------------------------------------------------------------------------------

ROOM_HALF = (2.5, 1.5, 3.0)
ANNEX_HALF = (1.0, 1.0, 1.0)
ANNEX_CENTRE = (4.5, 0.0, 0.0)                  # behind the room's x = +2.5 wall


def box_grid(half, centre=(0.0, 0.0, 0.0), cell=0.1):
    """The six flat faces of an axis-aligned box as vertex grids of `cell` metres, every cell split into two triangles ->
    (vertices float32 [V,3], faces int32 [F,3]).  Every face has its own grid (edges and corners repeat)."""
    verts, faces, base = [], [], 0
    for a in range(3):
        o = [k for k in range(3) if k != a]
        n0, n1 = int(round(2 * half[o[0]] / cell)), int(round(2 * half[o[1]] / cell))
        g0 = -half[o[0]] + cell * np.arange(n0 + 1)
        g1 = -half[o[1]] + cell * np.arange(n1 + 1)
        i0, i1 = np.meshgrid(np.arange(n0), np.arange(n1), indexing="ij")
        q = (i0 * (n1 + 1) + i1).reshape(-1)
        tri = np.concatenate([np.stack([q, q + n1 + 1, q + n1 + 2], 1), np.stack([q, q + n1 + 2, q + 1], 1)])
        for sgn in (-1.0, 1.0):
            p = np.zeros((n0 + 1, n1 + 1, 3))
            p[..., a] = sgn * half[a]
            p[..., o[0]] = g0[:, None]
            p[..., o[1]] = g1[None, :]
            verts.append(p.reshape(-1, 3) + np.asarray(centre, dtype=np.float64))
            faces.append(tri + base)
            base += (n0 + 1) * (n1 + 1)
    return np.concatenate(verts).astype(F32), np.concatenate(faces).astype(np.int32)


def room_and_annex():
    """The box room's walls, then the cube annex -> (vertices, faces, number of room vertices)."""
    rv, rf = box_grid(ROOM_HALF)
    av, af = box_grid(ANNEX_HALF, ANNEX_CENTRE)
    return np.concatenate([rv, av]), np.concatenate([rf, af + len(rv)]).astype(np.int32), len(rv)
