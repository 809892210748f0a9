"""Plain-numpy float32 restatement of the mesher (include/rtgs_slam.h, "meshing"): the per-voxel TSDF integration rule and
marching tetrahedra on the Freudenthal split, with the 16-case table generated here (not shared with csrc/tsdf.hip).  Used
only by tests; it is the definition the kernels are held to, bit for bit.  Also the mesh checks the CPU and GPU tests share
(manifoldness, Euler characteristic, signed volume, canonical form, box-room wall statistics)."""
import itertools
import math

import numpy as np

F = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# integration
# ---------------------------------------------------------------------------------------------------------------------

def new_volume(dims):
    """dims = (nx, ny, nz) -> tsdf [nz,ny,nx] = 1, weight = 0, rgb [3,nz,ny,nx] = 0."""
    nx, ny, nz = (int(d) for d in dims)
    return np.ones((nz, ny, nx), F), np.zeros((nz, ny, nx), F), np.zeros((3, nz, ny, nx), F)


def w2c_from_c2w(c2w):
    """The world-to-camera matrix as the product builds it: inverted in float64, then cast to float32."""
    return np.linalg.inv(np.asarray(c2w, dtype=np.float64)).astype(F)


def axis_centres(lo, n, voxel):
    return F(lo) + (np.arange(n, dtype=np.int64).astype(F) + F(0.5)) * F(voxel)


def integrate(tsdf, weight, rgb, lo, voxel, trunc, max_weight, depth, color, K, c2w):
    """One frame into the planes, in place.  depth [H,W], color [3,H,W] float32; K = (fx, fy, cx, cy)."""
    nz, ny, nx = tsdf.shape
    depth = np.ascontiguousarray(depth, dtype=F)
    color = np.ascontiguousarray(color, dtype=F)
    H, W = depth.shape
    fx, fy, cx, cy = (F(k) for k in K)
    trunc, max_weight = F(trunc), F(max_weight)
    M = w2c_from_c2w(c2w)
    x = axis_centres(lo[0], nx, voxel)[None, None, :]
    y = axis_centres(lo[1], ny, voxel)[None, :, None]
    z = axis_centres(lo[2], nz, voxel)[:, None, None]
    with np.errstate(all="ignore"):
        xc = ((M[0, 0] * x + M[0, 1] * y) + M[0, 2] * z) + M[0, 3]
        yc = ((M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z) + M[1, 3]
        zc = ((M[2, 0] * x + M[2, 1] * y) + M[2, 2] * z) + M[2, 3]
        assert xc.dtype == F and zc.dtype == F
        ok = zc > 0
        u = fx * xc / zc + cx
        v = fy * yc / zc + cy
        pu = np.floor(u + F(0.5))
        pv = np.floor(v + F(0.5))
        ok &= (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
    idx = np.nonzero(ok.reshape(-1))[0]
    px = pu.reshape(-1)[idx].astype(np.int64)
    py = pv.reshape(-1)[idx].astype(np.int64)
    d = depth[py, px]
    keep = d > 0
    idx, px, py, d = idx[keep], px[keep], py[keep], d[keep]
    sdf = d - zc.reshape(-1)[idx]
    keep = ~(sdf < -trunc)
    idx, px, py, sdf = idx[keep], px[keep], py[keep], sdf[keep]
    s = np.minimum(F(1), sdf / trunc)
    t, w = tsdf.reshape(-1), weight.reshape(-1)
    w0 = w[idx]
    w1 = w0 + F(1)
    t[idx] = (t[idx] * w0 + s) / w1
    c = rgb.reshape(3, -1)
    for ch in range(3):
        c[ch, idx] = (c[ch, idx] * w0 + color[ch, py, px]) / w1
    w[idx] = np.minimum(w1, max_weight)
    assert t.dtype == F and w.dtype == F
    return int(idx.size)


# ---------------------------------------------------------------------------------------------------------------------
# marching tetrahedra
# ---------------------------------------------------------------------------------------------------------------------

def _corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def make_tets():
    """The 6 tetrahedra around the main diagonal: corner codes (bit 0 = +x, 1 = +y, 2 = +z) along each axis permutation."""
    return [(0, 1 << a, (1 << a) | (1 << b), 7) for a, b, _ in itertools.permutations(range(3))]


def make_table():
    """table[t][m] = triangles of tetrahedron t when bit k of m says its k-th corner is inside: each triangle a tuple of 3
    edges (lower corner code, upper corner code), wound so that the normal points from the inside corners to the outside."""
    table = []
    for tet in make_tets():
        row = []
        for m in range(16):
            ins = [k for k in range(4) if (m >> k) & 1]
            outs = [k for k in range(4) if not (m >> k) & 1]
            if len(ins) in (0, 4):
                row.append(())
                continue
            if len(ins) == 1:
                tris = [[(ins[0], o) for o in outs]]
            elif len(ins) == 3:
                tris = [[(outs[0], i) for i in ins]]
            else:
                p, q = ins
                r, s = outs
                quad = [(p, r), (p, s), (q, s), (q, r)]
                tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
            towards = (np.mean([_corner_xyz(tet[k]) for k in outs], axis=0) - np.mean([_corner_xyz(tet[k]) for k in ins], axis=0))
            done = []
            for tri in tris:
                mid = [(_corner_xyz(tet[a]) + _corner_xyz(tet[b])) / 2 for a, b in tri]
                n = np.cross(mid[1] - mid[0], mid[2] - mid[0])
                assert abs(float(n @ towards)) > 1e-9
                if n @ towards < 0:
                    tri = [tri[0], tri[2], tri[1]]
                done.append(tuple((min(tet[a], tet[b]), max(tet[a], tet[b])) for a, b in tri))
            row.append(tuple(done))
        table.append(row)
    return table


def extract(tsdf, weight, rgb, lo, voxel, min_weight=1.0):
    """-> (vertices [V,3] f32, faces [F,3] int32, colors [V,3] f32, keys [V] int64): welded by key, vertices in key order,
    faces in (cell, tetrahedron, triangle) order."""
    nz, ny, nx = tsdf.shape
    tets, table = make_tets(), make_table()
    sub = lambda a, c: a[(c >> 2) & 1:nz - 1 + ((c >> 2) & 1), (c >> 1) & 1:ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]
    ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
    mask = np.zeros((nz - 1, ny - 1, nx - 1), np.int32)
    for c in range(8):
        ok &= sub(weight, c) >= F(min_weight)
        mask |= (sub(tsdf, c) < 0).astype(np.int32) << c
    act = ok & (mask > 0) & (mask < 255)
    iz, iy, ix = np.nonzero(act)
    mask = mask[act]
    lin = (iz.astype(np.int64) * ny + iy) * nx + ix
    t_flat, c_flat = tsdf.reshape(-1), rgb.reshape(3, -1)
    order, keys, pos, col = [], [], [], []
    for t, tet in enumerate(tets):
        case = np.zeros(mask.shape, np.int32)
        for k in range(4):
            case |= ((mask >> tet[k]) & 1) << k
        for m in range(1, 15):
            sel = np.nonzero(case == m)[0]
            if sel.size == 0:
                continue
            for j, tri in enumerate(table[t][m]):
                kk, pp, cc = [], [], []
                for a, b in tri:
                    off = lambda c: (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny
                    ia, ib = lin[sel] + off(a), lin[sel] + off(b)
                    ta, tb = t_flat[ia], t_flat[ib]
                    w = ta / (ta - tb)
                    p = []
                    for axis, i0 in enumerate((ix, iy, iz)):
                        pa = F(lo[axis]) + ((i0[sel] + ((a >> axis) & 1)).astype(F) + F(0.5)) * F(voxel)
                        pb = F(lo[axis]) + ((i0[sel] + ((b >> axis) & 1)).astype(F) + F(0.5)) * F(voxel)
                        p.append(pa + (pb - pa) * w)
                    kk.append(ia * 7 + ((a ^ b) - 1))
                    pp.append(np.stack(p, -1))
                    cc.append(np.stack([c_flat[ch, ia] + (c_flat[ch, ib] - c_flat[ch, ia]) * w for ch in range(3)], -1))
                order.append(np.stack([lin[sel], np.full(sel.size, t), np.full(sel.size, j)], -1))
                keys.append(np.stack(kk, -1))
                pos.append(np.stack(pp, 1))
                col.append(np.stack(cc, 1))
    if not keys:
        return np.zeros((0, 3), F), np.zeros((0, 3), np.int32), np.zeros((0, 3), F), np.zeros(0, np.int64)
    order, keys, pos, col = np.concatenate(order), np.concatenate(keys), np.concatenate(pos), np.concatenate(col)
    perm = np.lexsort((order[:, 2], order[:, 1], order[:, 0]))
    keys, pos, col = keys[perm].reshape(-1), pos[perm].reshape(-1, 3), col[perm].reshape(-1, 3)
    assert pos.dtype == F and col.dtype == F
    uk, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    return pos[first], inv.reshape(-1, 3).astype(np.int32), col[first], uk


# ---------------------------------------------------------------------------------------------------------------------
# inputs and checks shared by the tests
# ---------------------------------------------------------------------------------------------------------------------

SPHERE_R, SPHERE_H = 0.5, 0.04
SPHERE_CENTRE = (0.013, -0.007, 0.021)
SPHERE_LO, SPHERE_DIMS = (-0.8, -0.8, -0.8), (40, 40, 40)


def sphere_field():
    """The exact distance field of the sphere (positive outside) at the voxel centres, divided by trunc = 4 h and clipped to
    +-1; all weights 1; a smooth colour.  -> tsdf, weight, rgb."""
    nx, ny, nz = SPHERE_DIMS
    x = axis_centres(SPHERE_LO[0], nx, SPHERE_H).astype(np.float64)[None, None, :]
    y = axis_centres(SPHERE_LO[1], ny, SPHERE_H).astype(np.float64)[None, :, None]
    z = axis_centres(SPHERE_LO[2], nz, SPHERE_H).astype(np.float64)[:, None, None]
    cx, cy, cz = SPHERE_CENTRE
    d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - SPHERE_R
    tsdf = np.clip(d / (4 * SPHERE_H), -1.0, 1.0).astype(F)
    rgb = np.stack([0.5 + 0.4 * np.sin(3 * x + 0 * d), 0.5 + 0.4 * np.cos(2 * y + 0 * d), 0.5 + 0.4 * np.sin(z + 0 * d)]).astype(F)
    return tsdf, np.ones_like(tsdf), np.ascontiguousarray(rgb)


def sphere_eps():
    """Linear interpolation along an edge of length l <= L = sqrt(3) h of a field with unit gradient whose second derivative
    along the edge is at most 1 / (r - L) (every point of a crossed edge is at least r - L from the centre) misplaces the zero
    by at most l^2 / 8 * 1 / (r - L)."""
    L = math.sqrt(3.0) * SPHERE_H
    return L * L / (8.0 * (SPHERE_R - L))


def edge_use_counts(faces):
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return counts


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def check_sphere_mesh(vertices, faces):
    """The assertions of the sphere case: closed 2-manifold of genus 0, no degenerate face, every vertex within eps of the
    sphere, signed volume positive and within the bound.  Returns the measured figures."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    assert len(v) > 0 and len(f) > 0
    assert f.min() >= 0 and f.max() < len(v)
    assert len(np.unique(v, axis=0)) == len(v), "two vertices are equal"
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all(), "a face repeats an index"
    counts = edge_use_counts(f)
    assert (counts == 2).all(), f"edges used {np.unique(counts)} times"
    E = len(counts)
    assert len(v) - E + len(f) == 2, (len(v), E, len(f))
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    assert (area2 > 0).all(), "a face has no area"
    eps = sphere_eps()
    rounding = 1e-6                      # float32 positions of magnitude < 1 m: a few ulp of 6e-8
    dev = np.abs(np.linalg.norm(v - np.asarray(SPHERE_CENTRE), axis=1) - SPHERE_R)
    assert dev.max() <= eps + rounding, (dev.max(), eps)
    vol = signed_volume(v, f)
    vol0 = 4.0 * math.pi * SPHERE_R ** 3 / 3.0
    assert vol > 0
    # a closed surface between the spheres of radius r - eps and r + eps encloses a volume within
    # ((1 + eps / r)^3 - 1) = 3 eps / r + 3 (eps / r)^2 + (eps / r)^3 of the sphere's, relative
    q = eps / SPHERE_R
    bound = 3 * q + 3 * q * q + q ** 3
    rel = abs(vol / vol0 - 1.0)
    assert rel <= bound, (rel, bound)
    return {"V": len(v), "F": len(f), "E": E, "max_dev": float(dev.max()), "eps": eps, "volume_rel": rel, "volume_bound": bound}


def canonical(vertices, faces, colors, keys=None):
    """Vertices sorted by key (or, without keys, by (x, y, z) - unique after welding), faces remapped, every face rotated to
    start at its smallest index, faces sorted.  -> (vertices, faces, colors)."""
    v, f, c = np.asarray(vertices), np.asarray(faces, dtype=np.int64), np.asarray(colors)
    order = np.argsort(np.asarray(keys), kind="stable") if keys is not None else np.lexsort((v[:, 2], v[:, 1], v[:, 0]))
    rank = np.empty(len(v), np.int64)
    rank[order] = np.arange(len(v))
    f = rank[f]
    shift = np.argmin(f, axis=1)
    f = np.stack([f[np.arange(len(f)), (shift + k) % 3] for k in range(3)], -1)
    f = f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]
    return v[order], f, c[order]


BOX_HALF = (2.5, 1.5, 3.0)


def wall_stats(vertices, half=BOX_HALF, cell=0.1, near=0.15):
    """Distance of every vertex to the nearest wall plane of the box room (mean, 99th percentile, max, metres) and the share
    of the walls' area covered: the walls are cut into `cell`-sized squares, a square is covered when a vertex within `near`
    of its wall falls into it."""
    v = np.asarray(vertices, dtype=np.float64)
    h = np.asarray(half, dtype=np.float64)
    dist = np.abs(h[None, :] - np.abs(v))                    # to the nearer of the two walls of every axis
    ax = np.argmin(dist, axis=1)
    d = dist[np.arange(len(v)), ax]
    covered, total = 0, 0
    for a in range(3):
        o = [k for k in range(3) if k != a]
        n0, n1 = int(round(2 * h[o[0]] / cell)), int(round(2 * h[o[1]] / cell))
        for sgn in (-1.0, 1.0):
            sel = (ax == a) & (d < near) & (np.sign(v[:, a]) == sgn)
            i0 = np.clip(np.floor((v[sel, o[0]] + h[o[0]]) / cell).astype(np.int64), 0, n0 - 1)
            i1 = np.clip(np.floor((v[sel, o[1]] + h[o[1]]) / cell).astype(np.int64), 0, n1 - 1)
            covered += len(np.unique(i0 * n1 + i1))
            total += n0 * n1
    return {"mean": float(d.mean()), "p99": float(np.percentile(d, 99)), "max": float(d.max()), "covered": covered / total}


def box_room_case(n_frames=20):
    """The end-to-end case: a 240 x 320 camera (f = 200: a pixel is 1.5 cm wide at the far wall, under the 2 cm voxel) on
    synth.trajectory, the box room's depth and colour at the GT poses, and a 2 cm grid over the part of the room in front of
    the camera.  -> (cam, [(depth [H,W,1], colour [3,H,W], c2w float64 array)], lo, hi, voxel)."""
    from rtg_slam_amd import synth
    cam = synth.CameraSpec(240, 320, 200.0, 200.0, 159.5, 119.5)
    frames = []
    for p in synth.trajectory(n_frames, seed=11):
        d = synth.box_room_depth(cam, p)
        frames.append((d, synth.box_room_color(cam, p, d), p.numpy()))
    return cam, frames, (-2.6, -1.6, 1.0), (2.6, 1.6, 3.2), 0.02


def fuse_reference(cam, frames, lo, dims, voxel, trunc, max_weight=64.0):
    tsdf, weight, rgb = new_volume(dims)
    for depth, color, c2w in frames:
        integrate(tsdf, weight, rgb, lo, voxel, trunc, max_weight, np.asarray(depth, dtype=F).reshape(cam.H, cam.W),
                  np.asarray(color, dtype=F), (cam.fx, cam.fy, cam.cx, cam.cy), c2w)
    return tsdf, weight, rgb
