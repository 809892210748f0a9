"""Plain-numpy float32 restatement of the mesh texture bake (include/rtgs_slam.h, "mesh texture"; meshing.texture_mesh): the chart
level of every face, the Morton layout of the atlas, the texel-to-face map, the surface point of a texel, the bake of one view
and the finish.  Used only by tests; it is the definition the kernels of csrc/mesh_texture.hip are held to, bit for bit.  Every
float step is one correctly rounded float32 operation, in the order written here."""
import numpy as np

from tests import mesh_render_reference as rr
from tests.tsdf_reference import w2c_from_c2w

F32 = np.float32
MAX_LEVEL = 6
MAX_SIDE = 16384
UNASSIGNED, ASSIGNED, SEEN = 0, 1, 2


def _part1by1(v):
    v = np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    for sh, m in ((16, 0x0000FFFF0000FFFF), (8, 0x00FF00FF00FF00FF), (4, 0x0F0F0F0F0F0F0F0F), (2, 0x3333333333333333),
                  (1, 0x5555555555555555)):
        v = (v | (v << np.uint64(sh))) & np.uint64(m)
    return v


def _compact1by1(v):
    v = np.asarray(v, dtype=np.uint64) & np.uint64(0x5555555555555555)
    for sh, m in ((1, 0x3333333333333333), (2, 0x0F0F0F0F0F0F0F0F), (4, 0x00FF00FF00FF00FF), (8, 0x0000FFFF0000FFFF),
                  (16, 0x00000000FFFFFFFF)):
        v = (v | (v >> np.uint64(sh))) & np.uint64(m)
    return v


def morton_encode(x, y):
    """x goes to the even bits, y to the odd ones -> int64."""
    return (_part1by1(x) | (_part1by1(y) << np.uint64(1))).astype(np.int64)


def morton_decode(code):
    """-> (x, y) int64: the even and the odd bits of code."""
    c = np.asarray(code, dtype=np.int64).astype(np.uint64)
    return _compact1by1(c).astype(np.int64), _compact1by1(c >> np.uint64(1)).astype(np.int64)


def face_levels(vertices, faces, texel, max_level=MAX_LEVEL):
    """-> (levels int32 [F], capped int32 [F]).  A face's block is s = 2^l texels wide, l the smallest of 1..max_level with
    ((s - 1) texel)^2 >= its longest squared edge (float32, on squares); a longer face takes max_level and is capped; a face
    with a non-finite corner takes level 1."""
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    texel = F32(texel)
    A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all="ignore"):
        def d2(p, q):
            d = q - p
            return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        L = np.maximum(np.maximum(d2(A, B), d2(B, C)), d2(C, A))
        assert L.dtype == F32
        finite = np.isfinite(A).all(1) & np.isfinite(B).all(1) & np.isfinite(C).all(1)
        levels = np.zeros(len(f), dtype=np.int32)
        for l in range(1, max_level + 1):
            t = F32((1 << l) - 1) * texel
            levels[(levels == 0) & (t * t >= L)] = l
    capped = ((levels == 0) & finite).astype(np.int32)
    levels[levels == 0] = max_level
    levels[~finite] = 1
    return levels, capped


def atlas_size(T):
    """-> (Wt, Ht) for T texels of blocks: k the smallest integer with 4^k >= T, Wt = 2^k, Ht = 2^k when T > 2^(2k-1), else
    2^(k-1).  T = 0 gives (1, 1)."""
    T = int(T)
    if T == 0:
        return 1, 1
    k = 0
    while 4 ** k < T:
        k += 1
    return 1 << k, (1 << k) if 2 * T > 4 ** k else (1 << k) >> 1


def layout(levels):
    """Faces sorted by level descending (stable in the face index), the exclusive int64 prefix sum of 4^l over that order =
    the block's Morton code -> dict: order [F] (face of every sorted slot), sorted_offset [F] int64, offset [F] int64 (per
    face), origin [F,2] int32 (x0, y0), T, Wt, Ht."""
    levels = np.asarray(levels, dtype=np.int64)
    order = np.argsort(-levels, kind="stable")
    size = np.int64(4) ** levels[order]
    sorted_offset = np.cumsum(size) - size
    T = int(size.sum())
    offset = np.empty(len(levels), dtype=np.int64)
    offset[order] = sorted_offset
    x0, y0 = morton_decode(offset)
    Wt, Ht = atlas_size(T)
    return {"order": order.astype(np.int32), "sorted_offset": sorted_offset.astype(np.int64), "offset": offset,
            "origin": np.stack([x0, y0], 1).astype(np.int32).reshape(-1, 2), "T": T, "Wt": Wt, "Ht": Ht}


def texel_face(lay):
    """-> [Ht,Wt] int32: the face whose block holds the texel (the last sorted offset <= the texel's Morton code), -1 for codes
    >= T."""
    Ht, Wt = lay["Ht"], lay["Wt"]
    y, x = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    code = morton_encode(x, y)
    out = np.full((Ht, Wt), -1, dtype=np.int32)
    if len(lay["order"]):
        slot = np.searchsorted(lay["sorted_offset"], code, side="right") - 1
        ok = code < lay["T"]
        out[ok] = lay["order"][slot[ok]]
    return out


def face_uv(lay, levels):
    """-> [F,3,2] float32: the corners at the texel centres (x0 + 0.5, y0 + 0.5), (x0 + s - 0.5, y0 + 0.5), (x0 + 0.5,
    y0 + s - 0.5), divided by (Wt, Ht)."""
    o = lay["origin"].astype(F32)
    s = (np.int64(1) << np.asarray(levels, dtype=np.int64)).astype(F32)
    h = F32(0.5)
    Wt, Ht = F32(lay["Wt"]), F32(lay["Ht"])
    u0, v0 = (o[:, 0] + h) / Wt, (o[:, 1] + h) / Ht
    u1, v1 = ((o[:, 0] + s) - h) / Wt, ((o[:, 1] + s) - h) / Ht
    return np.stack([np.stack([u0, v0], 1), np.stack([u1, v0], 1), np.stack([u0, v1], 1)], 1).astype(F32).reshape(-1, 3, 2)


def texel_ab(tf, levels, lay):
    """-> (a, b) [Ht,Wt] float32 of every texel (0 where unassigned): i = x - x0, j = y - y0, mirrored across the hypotenuse
    when i + j > s - 1, (i, j) <- (s - 1 - j, s - 1 - i); a = i / (s - 1), b = j / (s - 1)."""
    Ht, Wt = tf.shape
    y, x = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    f = np.maximum(tf, 0).astype(np.int64)
    if len(levels) == 0:
        return np.zeros((Ht, Wt), F32), np.zeros((Ht, Wt), F32)
    s = np.int64(1) << np.asarray(levels, dtype=np.int64)[f]
    i, j = x - lay["origin"][f, 0], y - lay["origin"][f, 1]
    m = i + j > s - 1
    i, j = np.where(m, s - 1 - j, i), np.where(m, s - 1 - i, j)
    d = (s - 1).astype(F32)
    a, b = i.astype(F32) / d, j.astype(F32) / d
    a[tf < 0] = 0
    b[tf < 0] = 0
    return a, b


def _blend(pa, pb, pc, a, b):
    """(pa + a (pb - pa)) + b (pc - pa), per component."""
    return (pa + a[..., None] * (pb - pa)) + b[..., None] * (pc - pa)


def texel_points(vertices, faces, tf, a, b):
    """-> [Ht,Wt,3] float32: A + a (B - A) + b (C - A) of the texel's face (garbage where tf < 0)."""
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return np.zeros(tf.shape + (3,), F32)
    t = f[np.maximum(tf, 0)]
    with np.errstate(all="ignore"):
        return _blend(v[t[..., 0]], v[t[..., 1]], v[t[..., 2]], a, b)


def bake_view(acc, tf, a, b, vertices, faces, color, depth, K, c2w, tolerance, min_cos=0.2):
    """One view into acc [Ht,Wt,4] float32 (w r, w g, w b, w), in place -> the number of contributing texels.  color [3,H,W]
    float32, depth [H,W] float32 of this mesh at c2w (the camera in the mesh's frame), K = (fx, fy, cx, cy)."""
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    color = np.ascontiguousarray(color, dtype=F32)
    depth = np.ascontiguousarray(depth, dtype=F32).reshape(color.shape[1:])
    H, W = depth.shape
    fx, fy, cx, cy = (F32(k) for k in K)
    tolerance = F32(tolerance)
    min_cos2 = F32(min_cos) * F32(min_cos)
    M = w2c_from_c2w(c2w)
    O = np.asarray(c2w, dtype=np.float64).reshape(4, 4)[:3, 3].astype(F32)
    idx = np.nonzero(tf.reshape(-1) >= 0)[0]
    if idx.size == 0 or len(f) == 0:
        return 0
    t = f[tf.reshape(-1)[idx]]
    A, B, C = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    with np.errstate(all="ignore"):
        P = _blend(A, B, C, a.reshape(-1)[idx], b.reshape(-1)[idx])
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        xc = ((M[0, 0] * x + M[0, 1] * y) + M[0, 2] * z) + M[0, 3]
        yc = ((M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z) + M[1, 3]
        zc = ((M[2, 0] * x + M[2, 1] * y) + M[2, 2] * z) + M[2, 3]
        ok = zc > 0
        u = fx * xc / zc + cx
        vv = fy * yc / zc + cy
        x0, y0 = np.floor(u), np.floor(vv)
        ok &= (x0 >= 0) & (x0 <= F32(W - 2)) & (y0 >= 0) & (y0 <= F32(H - 2))
        pu, pv = np.floor(u + F32(0.5)), np.floor(vv + F32(0.5))
        keep = np.nonzero(ok)[0]
        d = depth[pv[keep].astype(np.int64), pu[keep].astype(np.int64)]
        good = (d > 0) & ~((zc[keep] - d) > tolerance)
        keep = keep[good]
        e1, e2 = B[keep] - A[keep], C[keep] - A[keep]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        r = O[None, :] - P[keep]
        dot = lambda p, q: (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]
        nr = dot(n, r)
        cos2 = (nr * nr) / (dot(n, n) * dot(r, r))
        assert cos2.dtype == F32
        good = cos2 >= min_cos2
        keep, cos2 = keep[good], cos2[good]
        zk = zc[keep]
        w = cos2 / (zk * zk)
        ix, iy = x0[keep].astype(np.int64), y0[keep].astype(np.int64)
        tx, ty = u[keep] - x0[keep], vv[keep] - y0[keep]
        flat = acc.reshape(-1, 4)
        rows = idx[keep]
        for c in range(3):
            img = color[c]
            c00, c10, c01, c11 = img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]
            top = c00 + tx * (c10 - c00)
            bot = c01 + tx * (c11 - c01)
            val = top + ty * (bot - top)
            flat[rows, c] = flat[rows, c] + w * val
        flat[rows, 3] = flat[rows, 3] + w
        assert w.dtype == F32 and val.dtype == F32
    return int(keep.size)


def finish(acc, tf, a, b, faces, colors):
    """-> (image [Ht,Wt,3] uint8, flags [Ht,Wt] uint8: 0 unassigned, 1 assigned and never seen, 2 seen).  Seen (w > 0): rgb / w;
    assigned only: (cA + a (cB - cA)) + b (cC - cA) of the face's vertex colours, 0.5 without colours; unassigned: 0.  Bytes are
    floor(c 255 + 0.5) clamped into 0..255 (NaN gives 0)."""
    Ht, Wt = tf.shape
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    col = np.zeros((Ht, Wt, 3), dtype=F32)
    assigned = tf >= 0
    w = acc[..., 3]
    seen = assigned & (w > 0)
    with np.errstate(all="ignore"):
        if colors is None or len(f) == 0:
            col[assigned] = F32(0.5)
        else:
            c = np.ascontiguousarray(colors, dtype=F32).reshape(-1, 3)
            t = f[tf[assigned]]
            col[assigned] = _blend(c[t[:, 0]], c[t[:, 1]], c[t[:, 2]], a[assigned], b[assigned])
        col[seen] = acc[..., :3][seen] / w[seen][:, None]
        q = np.floor(col * F32(255) + F32(0.5))
        assert q.dtype == F32
        q = np.fmin(np.fmax(q, F32(0)), F32(255))
    flags = np.where(seen, SEEN, np.where(assigned, ASSIGNED, UNASSIGNED)).astype(np.uint8)
    return q.astype(np.uint8), flags


def texture_mesh(vertices, faces, colors, K, H, W, views, texel, tolerance, max_level=MAX_LEVEL, min_cos=0.2, near=rr.NEAR,
                 depths=None):
    """The whole chain -> dict.  views: [(colour [3,H,W], c2w in the mesh's frame)]; the depth of view i is depths[i] when
    given, else the mesh rendered at c2w (mesh_render_reference.render).  "acc" holds a copy of the accumulators after
    every view."""
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    levels, capped = face_levels(v, f, texel, max_level)
    lay = layout(levels)
    if lay["Wt"] > MAX_SIDE:
        raise ValueError(f"{lay['T']} texels do not fit a {MAX_SIDE} x {MAX_SIDE} atlas")
    tf = texel_face(lay)
    a, b = texel_ab(tf, levels, lay)
    acc = np.zeros((lay["Ht"], lay["Wt"], 4), dtype=F32)
    after = []
    for i, (color, c2w) in enumerate(views):
        depth = depths[i] if depths is not None else rr.render(v, f.astype(np.int32), K, H, W, c2w, near)[0]
        bake_view(acc, tf, a, b, v, f, color, depth, K, c2w, tolerance, min_cos)
        after.append(acc.copy())
    image, flags = finish(acc, tf, a, b, f, colors)
    return {"levels": levels, "capped": capped, "layout": lay, "texel_face": tf, "a": a, "b": b, "uv": face_uv(lay, levels),
            "acc": after, "image": image, "flags": flags, "texels_assigned": int((flags >= ASSIGNED).sum()),
            "texels_seen": int((flags == SEEN).sum())}
