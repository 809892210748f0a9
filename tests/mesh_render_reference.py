"""Plain-numpy float32 restatement of the mesh renderer (include/rtgs_slam.h, "mesh render"; evaluation.MeshRenderer): the depth
and face maps of an indexed triangle mesh at a pinhole pose, the depth L1 of such a map, and the cull of what no pose saw.
Used only by tests; it is the definition the kernels of csrc/mesh_render.hip are held to, bit for bit.  Every float step is one
correctly rounded float32 operation, in the order written here.

Per vertex    the chain of visibility_reference.views_add: xc = ((m00 x + m01 y) + m02 z) + m03, yc and zc likewise, u = fx xc /
              zc + cx, v = fy yc / zc + cy, iz = 1 / zc.  Usable when zc > near (NaN fails).
Per face      dropped whole when a corner is not usable - there is NO clipping: a face that crosses the near plane leaves a
              hole.  Dropped too when one of its six u, v is not finite (an early exit: its edge values would be inf or NaN
              and cover nothing).  The box, in float: x0 = max(ceil(min u), 0), x1 = min(floor(max u), W - 1), y likewise;
              skipped unless x0 <= x1 and y0 <= y1; integers only after that.  Pixel centres are the integer coordinates.
Edge p -> q   E = (qu - pu) (py - pv) - (qv - pv) (px - pu), always evaluated with the endpoints in lexicographic (u, v) order
              and negated (exactly) when that reverses the edge: the two faces that share an edge see exact negatives, so a
              pixel centre on it belongs to at least one of them.  Endpoints with the same (u, v): the face is dropped.
              w0 = E(b, c), w1 = E(c, a), w2 = E(a, b), area = (w0 + w1) + w2.  Covered when all w >= 0 and area > 0, or all
              w <= 0 and area < 0: both windings render.
Depth         z = 1 / (((w0 iz_a + w1 iz_b) + w2 iz_c) / area), accepted when finite and > 0.
Resolve       every pixel keeps the smallest 64-bit key (bits(z) << 32) | face: the nearest surface, the lowest face index
              among equal depths, whatever order the faces come in.  depth 0 and face -1 where nothing was hit."""
import numpy as np

from tests import visibility_reference as vr
from tests.tsdf_reference import w2c_from_c2w

F32 = np.float32
NEAR = 0.05
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
_CHUNK = 1 << 21                                   # (face, pixel) pairs evaluated at once


def project(vertices, K, c2w, near=NEAR):
    """-> (u, v, iz [V] float32, usable [V] bool)."""
    p = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    fx, fy, cx, cy = (F32(k) for k in K)
    M = w2c_from_c2w(c2w)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        xc = ((M[0, 0] * x + M[0, 1] * y) + M[0, 2] * z) + M[0, 3]
        yc = ((M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z) + M[1, 3]
        zc = ((M[2, 0] * x + M[2, 1] * y) + M[2, 2] * z) + M[2, 3]
        u = fx * xc / zc + cx
        v = fy * yc / zc + cy
        iz = F32(1) / zc
    assert u.dtype == F32 and v.dtype == F32 and iz.dtype == F32
    return u, v, iz, zc > F32(near)


def _edge(pu, pv, qu, qv, px, py):
    """E of the directed edge p -> q at (px, py), per pair -> (E float32, degenerate bool)."""
    swap = (qu < pu) | ((qu == pu) & (qv < pv))
    su, sv = np.where(swap, qu, pu), np.where(swap, qv, pv)
    eu, ev = np.where(swap, pu, qu), np.where(swap, pv, qv)
    e = (eu - su) * (py - sv) - (ev - sv) * (px - su)
    assert e.dtype == F32
    return np.where(swap, -e, e), (pu == qu) & (pv == qv)


def render(vertices, faces, K, H, W, c2w, near=NEAR):
    """-> (depth [H,W] float32, face [H,W] int32) of the mesh seen from c2w (the camera in the mesh's frame)."""
    near = F32(near)
    assert near > 0
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    keys = np.full(H * W, EMPTY, dtype=np.uint64)
    with np.errstate(all="ignore"):
        u, v, iz, usable = project(vertices, K, c2w, near)
        fu, fv, fiz = u[f], v[f], iz[f]                                   # [F,3]
        ok = usable[f].all(axis=1) & np.isfinite(fu).all(axis=1) & np.isfinite(fv).all(axis=1)
        x0 = np.maximum(np.ceil(fu.min(axis=1)), F32(0))
        x1 = np.minimum(np.floor(fu.max(axis=1)), F32(W - 1))
        y0 = np.maximum(np.ceil(fv.min(axis=1)), F32(0))
        y1 = np.minimum(np.floor(fv.max(axis=1)), F32(H - 1))
        ok &= (x0 <= x1) & (y0 <= y1)
        idx = np.nonzero(ok)[0]
        ix0, iy0 = x0[idx].astype(np.int64), y0[idx].astype(np.int64)
        bw, bh = x1[idx].astype(np.int64) - ix0 + 1, y1[idx].astype(np.int64) - iy0 + 1
        n = bw * bh
        start = 0
        while start < len(idx):
            stop = start + max(1, int(np.searchsorted(np.cumsum(n[start:]), _CHUNK, side="right")))
            sl = slice(start, stop)
            start = stop
            rep = np.repeat(np.arange(sl.start, min(sl.stop, len(idx))), n[sl])
            first = np.cumsum(n[sl]) - n[sl]
            k = np.arange(len(rep)) - np.repeat(first, n[sl])               # row-major position inside the face's box
            ipx, ipy = ix0[rep] + k % bw[rep], iy0[rep] + k // bw[rep]
            px, py = ipx.astype(F32), ipy.astype(F32)
            fi = idx[rep]
            au, av, bu, bv, cu, cv = fu[fi, 0], fv[fi, 0], fu[fi, 1], fv[fi, 1], fu[fi, 2], fv[fi, 2]
            w0, d0 = _edge(bu, bv, cu, cv, px, py)
            w1, d1 = _edge(cu, cv, au, av, px, py)
            w2, d2 = _edge(au, av, bu, bv, px, py)
            area = (w0 + w1) + w2
            cover = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (area > 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0) & (area < 0))
            cover &= ~(d0 | d1 | d2)
            z = F32(1) / (((w0 * fiz[fi, 0] + w1 * fiz[fi, 1]) + w2 * fiz[fi, 2]) / area)
            assert z.dtype == F32
            cover &= np.isfinite(z) & (z > 0)
            key = (z[cover].view(np.uint32).astype(np.uint64) << np.uint64(32)) | fi[cover].astype(np.uint64)
            np.minimum.at(keys, (ipy * W + ipx)[cover], key)
    hit = keys != EMPTY
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F32), F32(0)).astype(F32)
    face = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return depth.reshape(H, W), face.reshape(H, W)


def depth_metrics(mesh_depth, ref_depth, min_depth, max_depth):
    """-> (valid_ratio, l1): valid where mesh_depth > 0 and min_depth < ref_depth < max_depth; the float64 mean of the float32
    |mesh_depth - ref_depth| over the valid pixels, 0 without any."""
    m = np.ascontiguousarray(mesh_depth, dtype=F32).reshape(-1)
    r = np.ascontiguousarray(ref_depth, dtype=F32).reshape(-1)
    valid = (m > 0) & (r > F32(min_depth)) & (r < F32(max_depth))
    n = int(valid.sum())
    with np.errstate(all="ignore"):
        diff = np.abs(m - r)
    assert diff.dtype == F32
    return n / m.size, (float(diff[valid].astype(np.float64).sum()) / n if n else 0.0)


def cull_unseen(vertices, faces, K, H, W, poses, tolerance, near=NEAR):
    """The faces whose three corners some pose saw -> (vertices, faces, views [V]): at every pose (c2w in the mesh's frame)
    the mesh is rendered, then its own vertices are tested against that render (visibility_reference.views_add)."""
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    views = np.zeros(len(v), np.int32)
    for c2w in poses:
        depth, _ = render(v, faces, K, H, W, c2w, near)
        vr.views_add(views, v, depth, K, c2w, tolerance)
    ov, of = vr.cull_mesh(v, faces, views, 1, False)
    return ov, of, views
