"""Plain-numpy restatement of the mesh registration (include/rtgs_slam.h, "mesh registration"; mesh_ops.register_to_mesh): the
gates of a correspondence, its float64 terms, the order in which rtgs_mesh_register_accumulate sums them, and the Gauss-Newton
loop around the nearest-face query.  Used only by tests; it is the definition csrc/mesh_register.hip and the host loop are held
to, bit for bit.  The query is the brute force of tests/mesh_distance_reference.py.

    gates    correspondence i takes part when 0 <= face[i] < F, d2[i] <= max_d2 in float32, the unit normal n of face[i]
             (mesh_distance_reference.face_unit_normals) is not (0, 0, 0) and, with source normals s, the float32
             |(s.x n.x + s.y n.y) + s.z n.z| >= min_cos.
    terms    float64, one rounded operation per step on the widened float32 inputs; a = the face's first corner:
             q = p - center, e = p - a, r = (n.x e.x + n.y e.y) + n.z e.z, J = (q x n, n),
             t = (J[i] J[j] for i <= j row-major: 21; J[i] r: 6; r r; d2; 1).  A correspondence that does not take part has t = +0.
    order    chunk i // 1024; slot s of a chunk starts at +0 and adds the points s, s + 256, s + 512, s + 768 of the chunk; the 256
             slots go through `tree`; the chunk values are added by slot s = chunk % 256 in ascending chunk order from +0 and go
             through `tree` again.
    tree     slots 64 w .. 64 w + 63 halve six times (x[l] += x[l + o], o = 32 .. 1), the four results give (w0 + w1) + (w2 + w3).
    loop     T (float64) starts at init; per iteration the ORIGINAL points go through float32(T) as rtgs_transform_map does
             (((T00 x + T01 y) + T02 z) + T03 in float32; source normals through the rotation with a translation of +0), the
             query, the sums; fewer than 6 inliers stop it; A x = -b through eigh with the directions lambda <= rank_tol
             lambda_max dropped; x = (w, v) is applied as the Rodrigues rotation by w and the translation v about the centre of
             the target's vertex box, from the left; it stops once |w| <= 1e-6 and |v| <= 1e-6, or after max_iterations updates."""
import numpy as np

from tests import mesh_distance_reference as mdr

F32, F64 = np.float32, np.float64
CHUNK, SLOTS, WAVE, OUT = 1024, 256, 64, 30
STOP = 1e-6
MIN_INLIERS = 6


def box_center(vertices, faces):
    """The centre of the box of the vertices the faces use: float64 mean of the float32 corners, rounded to float32."""
    v, f = mdr._mesh(vertices, faces)
    used = v[f.reshape(-1)]
    return ((used.min(0).astype(F64) + used.max(0).astype(F64)) * 0.5).astype(F32)


def takes_part(face, d2, normals_hit, max_d2, src_normals=None, min_cos=0.0, F=None):
    face = np.asarray(face, dtype=np.int64)
    d2 = np.asarray(d2, dtype=F32)
    ok = (face >= 0) & (d2 <= F32(max_d2)) & (normals_hit != 0).any(axis=1)
    if F is not None:
        ok &= face < F
    if src_normals is not None:
        s = np.asarray(src_normals, dtype=F32)
        dot = (s[:, 0] * normals_hit[:, 0] + s[:, 1] * normals_hit[:, 1]) + s[:, 2] * normals_hit[:, 2]
        assert dot.dtype == F32
        ok &= np.abs(dot) >= F32(min_cos)
    return ok


def terms(points, face, d2, vertices, faces, center, max_d2, src_normals=None, min_cos=0.0):
    """-> [N, 30] float64: the terms of every correspondence, +0 rows for those that do not take part."""
    v, f = mdr._mesh(vertices, faces)
    p32 = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    face = np.asarray(face, dtype=np.int64).reshape(-1)
    d2 = np.asarray(d2, dtype=F32).reshape(-1)
    N = len(p32)
    safe = np.where((face >= 0) & (face < len(f)), face, 0)
    n32 = mdr.face_unit_normals(v, f)[safe]
    n32[(face < 0) | (face >= len(f))] = 0
    ok = takes_part(face, d2, n32, max_d2, src_normals, min_cos, len(f))
    p, n, a = p32.astype(F64), n32.astype(F64), v[f[safe, 0]].astype(F64)
    q = p - np.asarray(center, dtype=F32).astype(F64)
    e = p - a
    r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
    J = np.stack([q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1], q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2], q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0],
                  n[:, 0], n[:, 1], n[:, 2]], axis=1)
    t = np.zeros((N, OUT), F64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            t[:, k] = J[:, i] * J[:, j]
            k += 1
    for i in range(6):
        t[:, 21 + i] = J[:, i] * r
    t[:, 27] = r * r
    t[:, 28] = d2.astype(F64)
    t[:, 29] = 1.0
    t[~ok] = 0.0
    return t


def tree(x):
    """[..., 256, K] -> [..., K]."""
    w = x.reshape(x.shape[:-2] + (SLOTS // WAVE, WAVE, x.shape[-1]))
    o = WAVE // 2
    while o >= 1:
        w = w[..., :o, :] + w[..., o:2 * o, :]
        o //= 2
    w = w[..., 0, :]
    return (w[..., 0, :] + w[..., 1, :]) + (w[..., 2, :] + w[..., 3, :])


def _slots(rows):
    """[R, K] -> [256, K]: slot s starts at +0 and adds the rows s, s + 256, ... in order."""
    R, K = rows.shape
    groups = -(-R // SLOTS)
    padded = np.zeros((groups * SLOTS, K), F64)
    padded[:R] = rows
    acc = np.zeros((SLOTS, K), F64)
    for g in padded.reshape(groups, SLOTS, K):
        acc = acc + g
    return acc


def ordered_sum(t):
    """[N, K] float64 -> [K]: the sum in the kernel's order."""
    N, K = t.shape
    chunks = -(-N // CHUNK)
    padded = np.zeros((chunks * CHUNK, K), F64)
    padded[:N] = t
    padded = padded.reshape(chunks, CHUNK // SLOTS, SLOTS, K)
    acc = np.zeros((chunks, SLOTS, K), F64)
    for step in range(CHUNK // SLOTS):
        acc = acc + padded[:, step]
    return tree(_slots(tree(acc).reshape(chunks, K)))


def accumulate(points, face, d2, vertices, faces, center, max_d2, src_normals=None, min_cos=0.0):
    """rtgs_mesh_register_accumulate -> out [30] float64."""
    return ordered_sum(terms(points, face, d2, vertices, faces, center, max_d2, src_normals, min_cos))


def normal_matrix(out):
    A = np.zeros((6, 6), F64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = out[k]
            k += 1
    return A, np.array(out[21:27], dtype=F64)


def solve(out, rank_tol=1e-8):
    """-> (x, rank, eigenvalues ascending, eigenvectors as columns): x = - sum over the kept j of e_j (e_j . b) / lambda_j, added in
    ascending j from 0."""
    A, b = normal_matrix(out)
    lam, E = np.linalg.eigh(A)
    x = np.zeros(6, F64)
    rank = 0
    for j in range(6):
        if lam[j] > rank_tol * lam[5]:
            x = x - E[:, j] * (np.dot(E[:, j], b) / lam[j])
            rank += 1
    return x, rank, lam, E


def rodrigues(w):
    th = np.sqrt(np.dot(w, w))
    if not th > 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def twist_matrix(x, center):
    """The 4x4 of x = (w, v) about `center`: p -> R (p - c) + c + v."""
    c = np.asarray(center, dtype=F32).astype(F64)
    D = np.eye(4)
    D[:3, :3] = rodrigues(x[:3])
    D[:3, 3] = (c + x[3:]) - D[:3, :3] @ c
    return D


def transform_f32(points, T, translate=True):
    """rtgs_transform_map with float32(T); translate False: the translation column is +0."""
    m = np.asarray(T, dtype=F64).astype(F32)
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    cols = []
    for r in range(3):
        t = m[r, 3] if translate else F32(0)
        cols.append(((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + t)
    out = np.stack(cols, axis=1)
    assert out.dtype == F32
    return out


def register(points, vertices, faces, max_distance=0.10, max_iterations=30, source_normals=None, min_cos=0.0, init=None,
             rank_tol=1e-8):
    """-> (T [4,4] float64, report): iterations, converged, reason, inliers, rank, rms_plane_before / _after,
    rms_distance_before / _after, and "twists": every x applied."""
    v, f = mdr._mesh(vertices, faces)
    p0 = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    center = box_center(v, f)
    md = F32(max_distance)
    max_d2 = md * md
    assert max_d2.dtype == F32
    T = np.eye(4) if init is None else np.array(init, dtype=F64).reshape(4, 4)
    rep = {"iterations": 0, "converged": False, "reason": "max iterations", "inliers": [], "rank": 0, "twists": []}
    first = last = None
    while True:
        moved = transform_f32(p0, T)
        sn = None if source_normals is None else transform_f32(source_normals, T, translate=False)
        d2, face = mdr.nearest(moved, v, f)
        out = accumulate(moved, face, d2, v, f, center, max_d2, sn, min_cos)
        count = int(out[29])
        rep["inliers"].append(count)
        last = out
        first = out if first is None else first
        if count < MIN_INLIERS:
            rep["reason"] = "too few inliers"
            break
        x, rep["rank"], _, _ = solve(out, rank_tol)
        T = twist_matrix(x, center) @ T
        rep["twists"].append(x)
        rep["iterations"] += 1
        if np.sqrt(np.dot(x[:3], x[:3])) <= STOP and np.sqrt(np.dot(x[3:], x[3:])) <= STOP:
            rep["converged"], rep["reason"] = True, "converged"
            break
        if rep["iterations"] >= max_iterations:
            break
    for name, o in (("before", first), ("after", last)):
        n = o[29]
        rep["rms_plane_" + name] = float(np.sqrt(o[27] / n)) if n else float("nan")
        rep["rms_distance_" + name] = float(np.sqrt(o[28] / n)) if n else float("nan")
    return T, rep


# ---- the shapes and sources the CPU and GPU tests share ----

def rigid(axis, degrees, translation):
    """The 4x4 of a rotation by `degrees` about `axis` through the origin, then `translation`."""
    a = np.asarray(axis, dtype=F64)
    T = np.eye(4)
    T[:3, :3] = rodrigues(a / np.linalg.norm(a) * np.deg2rad(degrees))
    T[:3, 3] = translation
    return T


def voxel_shell(occupied, spacing, origin):
    """The closed boundary of a set of grid cells -> (vertices float32, faces int32): one quad, two faces, per cell side that
    borders an empty cell; corners shared."""
    occ = np.pad(np.asarray(occupied, dtype=bool), 1)
    index, verts, faces = {}, [], []

    def vid(c):
        if c not in index:
            index[c] = len(verts)
            verts.append([origin[k] + spacing[k] * c[k] for k in range(3)])
        return index[c]

    for x, y, z in zip(*np.nonzero(occ)):
        for axis in range(3):
            for side in (0, 1):
                nb = [x, y, z]
                nb[axis] += 2 * side - 1
                if occ[tuple(nb)]:
                    continue
                u, w = (axis + 1) % 3, (axis + 2) % 3
                quad = []
                for du, dw in ((0, 0), (1, 0), (1, 1), (0, 1)):
                    c = [x - 1, y - 1, z - 1]
                    c[axis] += side
                    c[u] += du
                    c[w] += dw
                    quad.append(vid(tuple(int(i) for i in c)))
                if not side:
                    quad = quad[::-1]
                faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return np.asarray(verts, dtype=F32), np.asarray(faces, dtype=np.int32)


def room():
    """An L-shaped room with a step: 8 x 6 x 3 cells of 0.25 x 0.25 x 0.3 m around the origin, a quadrant cut out of the L, the
    floor raised by one cell along one wall.  Closed, without a symmetry; every vertex within 1.5 m of the box centre."""
    occ = np.ones((8, 6, 3), bool)
    occ[4:, 3:, :] = False
    occ[:2, :, 0] = False
    return voxel_shell(occ, (0.25, 0.25, 0.3), (-1.0, -0.75, -0.45))


def wall():
    """A square wall of 2 x 2 quads (8 faces) of 1 m, in a general orientation."""
    xs = np.array([-1.0, 0.0, 1.0])
    v = np.array([[x, y, 0.0] for y in xs for x in xs])
    f = []
    for j in range(2):
        for i in range(2):
            a, b, c, d = j * 3 + i, j * 3 + i + 1, (j + 1) * 3 + i + 1, (j + 1) * 3 + i
            f += [(a, b, c), (a, c, d)]
    R = rigid((0.3, -0.5, 0.8), 37.0, (0.2, -0.1, 0.4))
    v = v @ R[:3, :3].T + R[:3, 3]
    return v.astype(F32), np.asarray(f, dtype=np.int32)


def sample(vertices, faces, n, seed):
    """n points on the faces, by area then uniform -> (points float64 [n,3], own face int32 [n])."""
    v, f = mdr._mesh(vertices, faces)
    rng = np.random.default_rng(seed)
    a, b, c = (v[f[:, k]].astype(F64) for k in range(3))
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    own = rng.choice(len(f), n, p=area / area.sum())
    uv = rng.random((n, 2))
    flip = uv.sum(1) > 1
    uv[flip] = 1 - uv[flip]
    return a[own] + uv[:, :1] * (b[own] - a[own]) + uv[:, 1:] * (c[own] - a[own]), own.astype(np.int32)


def apply(T, p):
    return np.asarray(p, dtype=F64) @ T[:3, :3].T + T[:3, 3]


KNOWN = rigid((0.4, -0.7, 0.59), 1.5, np.array([0.6, -0.5, 0.62]) / np.linalg.norm([0.6, -0.5, 0.62]) * 0.027)


def room_case(n=2000, seed=11):
    """-> (source float32 [n,3], own-face unit normals of the source in ITS frame float32, vertices, faces, KNOWN): n samples of
    the room moved by inverse(KNOWN), so that register() should return KNOWN."""
    v, f = room()
    p, own = sample(v, f, n, seed)
    inv = np.linalg.inv(KNOWN)
    src = apply(inv, p).astype(F32)
    nrm = (mdr.face_unit_normals(v, f)[own].astype(F64) @ inv[:3, :3].T).astype(F32)
    return src, nrm, v, f, KNOWN


def room_outliers(src, n_out, seed=12):
    """n_out points 0.5 m above the room's box, spread between the rows of src -> (points, mask of the outliers)."""
    v, _ = room()
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    out = np.stack([rng.uniform(lo[0], hi[0], n_out), rng.uniform(lo[1], hi[1], n_out), np.full(n_out, hi[2] + 0.5)], axis=1)
    out = apply(np.linalg.inv(KNOWN), out).astype(F32)
    n = len(src) + n_out
    mask = np.zeros(n, bool)
    mask[rng.choice(n, n_out, replace=False)] = True
    pts = np.empty((n, 3), F32)
    pts[mask], pts[~mask] = out, src
    return pts, mask


def wall_case(n=500, seed=13):
    """-> (source float32, vertices, faces): samples of the wall tilted by 0.5 degrees about an in-plane axis through its centre
    and offset 1 cm along its normal."""
    v, f = wall()
    p, _ = sample(v, f, n, seed)
    nrm = mdr.face_unit_normals(v, f)[0].astype(F64)
    c = box_center(v, f).astype(F64)
    inplane = (v[1] - v[0]).astype(F64)
    R = rodrigues(inplane / np.linalg.norm(inplane) * np.deg2rad(0.5))
    return ((p - c) @ R.T + c + 0.01 * nrm).astype(F32), v, f
