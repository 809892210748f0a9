"""Plain-numpy restatement of the point-to-mesh distance (include/rtgs_slam.h, "mesh distance"; mesh_ops.MeshDistance): the
float32 squared distance from a point to one triangle, the brute-force nearest face over ALL faces, and the unit normal of
the hit face.  Used only by tests; it is the definition the kernels of csrc/mesh_distance.hip are held to, bit for bit.  No
acceleration structure appears here, and the kernels' result must not depend on theirs.

Every step is one correctly rounded float32 operation in the order written (the kernel file is built with
-ffp-contract=off).  dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z.  clamp01(t) = t > 0 ? (t < 1 ? t : 1) : 0, so a NaN gives 0.

    seg(p, s, e)          d = e - s, w = p - s, dd = dot(d, d), t = dd > 0 ? clamp01(dot(w, d) / dd) : 0,
                          q = w - t d, the value is dot(q, q).  The ends are ordered by VERTEX INDEX, lower first, so the edge
                          two faces share gives both the same bits.
    interior(p, a, b, c)  ab = b - a, ac = c - a, w = p - a, abab = dot(ab, ab), acac = dot(ac, ac), abac = dot(ab, ac),
                          det = abab acac - abac abac; it takes part only when det > 0.  d1 = dot(w, ab), d2 = dot(w, ac),
                          s = clamp01((d1 acac - d2 abac) / det), r = 1 - s, t = (d2 abab - d1 abac) / det,
                          t = t > 0 ? (t < r ? t : r) : 0, q = (w - s ab) - t ac, the value is dot(q, q).
    pair_d2               the minimum of the three seg values (edges ab, bc, ca) and, where it takes part, of interior.

Why the interior is the clamped-barycentric form and not the plane form ((p - a) . n)^2 / n.n behind three sign tests: every
candidate above is the distance from p to a point a + s ab + t ac with (s, t) inside the triangle, WHATEVER s and t came out
as.  So each is at least the true distance minus a rounding term that depends only on the coordinates' magnitude, never on
the triangle's conditioning - the bound the grid query's stopping rule needs ("mesh distance").  The plane form
has no such bound: the normal of a needle face is rounding noise, and its candidate can be arbitrarily small far away.

Properties (tests/test_mesh_distance_cpu.py): finite and never NaN for |coordinate| <= 2^20 (MeshDistance refuses vertices
beyond that); exactly 0 for a point bit-equal to a corner; exactly h h at a power-of-two height h above the interior of an
axis-aligned face with power-of-two coordinates and legs along the axes from corner a (s and t are then exact), and above
a well-shaped axis-aligned face of extent L when h >= L / 64 (q.z = h exactly, and the in-plane residue of q, a few ulps of
L, squares to less than half an ulp of h h)."""
import numpy as np

F32 = np.float32
MAX_COORD = float(2 ** 20)


def _f(x):
    x = np.asarray(x, dtype=F32)
    assert x.dtype == F32
    return x


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _clamp01(t):
    return np.where(t > 0, np.where(t < 1, t, F32(1)), F32(0)).astype(F32)


def seg(p, s, e):
    p, s, e = _f(p), _f(s), _f(e)
    d, w = e - s, p - s
    dd = _dot(d, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dd > 0, _clamp01(_dot(w, d) / dd), F32(0)).astype(F32)
    q = w - t[..., None] * d
    out = _dot(q, q)
    assert out.dtype == F32
    return out


def interior(p, a, b, c):
    """-> (value, takes_part)."""
    p, a, b, c = _f(p), _f(a), _f(b), _f(c)
    ab, ac, w = b - a, c - a, p - a
    abab, acac, abac = _dot(ab, ab), _dot(ac, ac), _dot(ab, ac)
    det = abab * acac - abac * abac
    d1, d2 = _dot(w, ab), _dot(w, ac)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = _clamp01((d1 * acac - d2 * abac) / det)
        t = (d2 * abab - d1 * abac) / det
    r = F32(1) - s
    t = np.where(t > 0, np.where(t < r, t, r), F32(0)).astype(F32)
    q = (w - s[..., None] * ab) - t[..., None] * ac
    out = _dot(q, q)
    assert out.dtype == F32
    return out, det > 0


def pair_d2(p, a, b, c, ia=0, ib=1, ic=2):
    """The float32 squared distance from p to the triangle a b c whose corners have the vertex indices ia, ib, ic (they order
    the ends of each edge).  Broadcasts over leading dimensions."""
    p, a, b, c = _f(p), _f(a), _f(b), _f(c)
    ia, ib, ic = (np.asarray(i)[..., None] for i in (ia, ib, ic))

    def edge(u, iu, v, iv):
        sw = iv < iu
        return seg(p, np.where(sw, v, u), np.where(sw, u, v))

    m = np.minimum(np.minimum(edge(a, ia, b, ib), edge(b, ib, c, ic)), edge(c, ic, a, ia))
    v, ok = interior(p, a, b, c)
    return np.where(ok & (v < m), v, m).astype(F32)


def _mesh(vertices, faces):
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    assert f.shape[0] > 0 and f.min() >= 0 and f.max() < len(v)
    return v, f


def nearest(points, vertices, faces, chunk=256):
    """-> (d2 float32 [N], face int32 [N]): d2[i] = the minimum of pair_d2 over ALL faces, face[i] = the lowest face index
    that attains it; a point with a non-finite coordinate gives (inf, -1).  Brute force, vectorised over the faces."""
    v, f = _mesh(vertices, faces)
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    ia, ib, ic = f[:, 0][None], f[:, 1][None], f[:, 2][None]
    d2 = np.full(len(p), np.inf, F32)
    face = np.full(len(p), -1, np.int32)
    ok = np.isfinite(p).all(axis=1)
    idx = np.nonzero(ok)[0]
    for lo in range(0, len(idx), chunk):
        sel = idx[lo:lo + chunk]
        d = pair_d2(p[sel][:, None, :], a, b, c, ia, ib, ic)            # [chunk, F]
        k = np.argmin(d, axis=1)                                       # the first, so the lowest, index of the minimum
        d2[sel] = d[np.arange(len(sel)), k]
        face[sel] = k.astype(np.int32)
    return d2, face


def face_unit_normals(vertices, faces):
    """[F,3] float32: n = (b - a) x (c - a) as mesh_ops_reference.face_normals (every component two rounded products and a
    rounded difference), divided by l = sqrt((x x + y y) + z z) when l > 0 and finite, (0, 0, 0) otherwise."""
    v, f = _mesh(vertices, faces)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                  e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    l = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    assert n.dtype == F32 and l.dtype == F32
    ok = (l > 0) & np.isfinite(l)
    out = np.zeros_like(n)
    out[ok] = n[ok] / l[ok, None]
    return out


def hit_normals(vertices, faces, face):
    """[N,3] float32: face_unit_normals of face[i], (0, 0, 0) where face[i] < 0."""
    fn = face_unit_normals(vertices, faces)
    face = np.asarray(face, dtype=np.int64).reshape(-1)
    out = np.zeros((len(face), 3), F32)
    out[face >= 0] = fn[face[face >= 0]]
    return out


def normal_consistency(n_own, n_hit):
    """-> (float64 sum of |dot(n_own, n_hit)| over the counted samples, their number): the dot and the absolute value in
    float32, the sum in float64; a sample whose own or hit normal is (0, 0, 0) - a degenerate face - is counted out."""
    n_own, n_hit = _f(n_own), _f(n_hit)
    ok = (n_own != 0).any(axis=1) & (n_hit != 0).any(axis=1)
    d = np.abs(_dot(n_own, n_hit))
    return float(d[ok].astype(np.float64).sum()), int(ok.sum())


def eval_mesh_surface(rec_samples, rec_own_face, rec_v, rec_f, gt_samples, gt_own_face, gt_v, gt_f, dist_thres=(0.03,)):
    """The composition evaluation.eval_mesh_surface is held to, on given samples (float32 [N,3] with the face each was drawn
    on): accuracy / precision from the reconstruction's samples to the GT surface, completion / recall from the GT's samples
    to the reconstruction's surface, the keys of eval_pcd, and the normal consistencies.  Sums are float64."""
    res = {}
    sides = (("acc", rec_samples, rec_own_face, rec_v, rec_f, gt_v, gt_f), ("comp", gt_samples, gt_own_face, gt_v, gt_f, rec_v, rec_f))
    frac = {}
    for name, pts, own, ov, of, tv, tf in sides:
        d2, face = nearest(pts, tv, tf)
        d = np.sqrt(d2.astype(np.float64))                            # as rtgs_eval_nn_stats: the float32 d2, its root in float64
        n = len(d)
        res["accuracy" if name == "acc" else "completion"] = float(d.sum()) / n * 100.0
        frac[name] = [float((d < t).sum()) / n * 100.0 for t in dist_thres]
        s, cnt = normal_consistency(hit_normals(ov, of, own), hit_normals(tv, tf, face))
        res["normal_consistency_" + name] = s / cnt if cnt else float("nan")
        res["normal_samples_" + name] = cnt
    for j, t in enumerate(dist_thres):
        P, R = frac["acc"][j], frac["comp"][j]
        res[f"P (< {t})"], res[f"R (< {t})"] = P, R
        res[f"F1 (< {t})"] = 2 * P * R / (P + R) if P + R > 0 else float("nan")
    res["normal_consistency"] = 0.5 * (res["normal_consistency_acc"] + res["normal_consistency_comp"])
    return res


# ---- an independent float64 closest point on a triangle (Ericson, Real-Time Collision Detection 5.1.5: the region form) ----

def closest_point_f64(p, a, b, c):
    p, a, b, c = (np.asarray(x, dtype=np.float64) for x in (p, a, b, c))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        return a
    bp = p - b
    d3, d4 = ab @ bp, ac @ bp
    if d3 >= 0 and d4 <= d3:
        return b
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return a + (d1 / (d1 - d3)) * ab
    cp = p - c
    d5, d6 = ab @ cp, ac @ cp
    if d6 >= 0 and d5 <= d6:
        return c
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return a + (d2 / (d2 - d6)) * ac
    va = d3 * d6 - d5 * d4
    if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        return b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (c - b)
    den = 1.0 / (va + vb + vc)
    return a + ab * (vb * den) + ac * (vc * den)


def distance_f64(p, a, b, c):
    q = closest_point_f64(p, a, b, c)
    return float(np.linalg.norm(np.asarray(p, dtype=np.float64) - q))


# ---- the meshes and points the CPU and GPU tests share ----

def soup(F, seed, box=4.0):
    """F triangles, 3 F vertices of their own plus a few shared ones: mostly small (edge ~ box / 40), every 16th spans a good
    part of the box, so that at the default cell some faces take the wave path; coordinates within +-box."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.8 * box, 0.8 * box, (F, 1, 3))
    size = np.where(np.arange(F) % 16 == 7, 0.2 * box, box / 40.0)[:, None, None]
    v = (centre + rng.uniform(-1, 1, (F, 3, 3)) * size).astype(F32).reshape(-1, 3)
    v = np.clip(v, -box, box)
    f = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    if F >= 4:                                     # two faces share an edge, one repeats a corner of another
        f[1, 0], f[1, 1] = f[0, 1], f[0, 0]
        f[3, 2] = f[2, 2]
    return v, f


def soup_points(v, f, n, seed):
    """n points in four equal parts: uniform in the mesh's box, on faces (from barycentrics), outside the box by up to half its
    extent, and 100 x the extent away."""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ext = float((hi - lo).max()) or 1.0
    k = n // 4
    inside = rng.uniform(lo, hi, (k, 3))
    fi = rng.integers(0, len(f), k)
    uv = rng.random((k, 2))
    flip = uv.sum(1) > 1
    uv[flip] = 1 - uv[flip]
    a, b, c = (v[f[fi, j]].astype(np.float64) for j in range(3))
    on = a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a)
    out = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (k, 3))
    far = rng.normal(size=(n - 3 * k, 3))
    far = 100.0 * ext * far / np.linalg.norm(far, axis=1, keepdims=True) + 0.5 * (lo + hi)
    return np.concatenate([inside, on, out, far]).astype(F32)


def lattice(n=16, spacing=0.25):
    """A planar n x n lattice of squares in z = 0 from the origin, each split into two faces; spacing a power of two."""
    xs = np.arange(n + 1, dtype=np.float64) * spacing
    gx, gy = np.meshgrid(xs, xs, indexing="xy")
    v = np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros((n + 1) ** 2)], axis=1).astype(F32)
    idx = lambda i, j: j * (n + 1) + i
    f = []
    for j in range(n):
        for i in range(n):
            f.append((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)))
            f.append((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))
    return v, np.asarray(f, dtype=np.int32)


def lattice_points(n=16, spacing=0.25):
    """Points exactly equidistant from several faces: above every inner lattice vertex (6 faces meet there) and above the
    midpoints of the inner edges (2 faces), at power-of-two heights."""
    pts = []
    for h in (0.0, 0.125, 0.5, 2.0):
        for j in range(1, n):
            for i in range(1, n):
                pts.append((i * spacing, j * spacing, h))
                pts.append(((i + 0.5) * spacing, j * spacing, h))
                pts.append((i * spacing, (j + 0.5) * spacing, -h))
    return np.asarray(pts, dtype=F32)


def hand_made():
    """Sound faces, duplicates and the three kinds of degenerate face (two equal corners, three equal corners, collinear
    corners) in one mesh -> (vertices, faces)."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, -5], [2, 2, 2], [3, 3, 3], [4, 4, 4], [0.5, 0.5, -1]], F32)
    f = np.array([[0, 1, 2], [1, 3, 2], [0, 1, 2], [2, 1, 0], [0, 0, 1], [4, 4, 4], [5, 6, 7], [0, 1, 8], [1, 3, 2]], np.int32)
    return v, f
