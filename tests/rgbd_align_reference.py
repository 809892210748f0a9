"""Plain-numpy restatement of the RGB-D pose refinement (include/rtgs_icp.h, "RGB-D refinement"; rtg_slam_amd/rgbd_align.py):
the intensity pyramid, the gates of a source pixel, its float32 geometric and photometric terms, the order in which
rtgs_rgbd_align_accumulate sums them in float64, and the Gauss-Newton loop.  Used only by tests; it is the definition
csrc/rgbd_align.hip and the host loop are held to, bit for bit.  Conventions are rtgs_icp_step's: `pose` (4x4 float32) maps
source (current frame, t1) points into the target (last frame / model, t0) camera, K is the level's, maps are [H,W,3] / [H,W],
the Jacobian is ordered (rotation, translation), the update is T <- exp(x) T.

    pyramid  grey = (0.299 R + 0.587 G) + 0.114 B; level l of L has size (H >> (L-1-l), W >> (L-1-l)); a coarser level is
             ((a + b) + (c + d)) * 0.25 over the 2 x 2 block at (2y, 2x) of the next finer one (a b the upper row); float32.
    pixel    every float32 step is one rounded operation.  p = source vertex, q = R p + t as ((r0 x + r1 y) + r2 z) + t,
             u = (q.x / q.z) fx + cx, v likewise; in view: 0 < u < W-1 and 0 < v < H-1 (a NaN fails).
             nearest pixel (rtgs_icp_step's: grid_sample nearest, align_corners): hw = (W-1) / 2, ix = (((u / hw - 1) + 1) / 2)
             (W-1) clamped to [0, W-1], rounded half to even; iy likewise; g, m = target vertex, normal there.
             photometric gate: in view, p.z > 0, q.z > 0, g.z > 0, e = q - g, sqrt((e.x e.x + e.y e.y) + e.z e.z) <= distance.
             geometric gate: the photometric gate and (Rn.x m.x + Rn.y m.y) + Rn.z m.z > cos, Rn = (r0 n.x + r1 n.y) + r2 n.z.
             r_G = (m.x e.x + m.y e.y) + m.z e.z, J_G = (q x m, m), cross products as a.y b.z - a.z b.y.
             x0 = floor(u), y0 = floor(v), a = u - x0, b = v - y0, i00 i10 i01 i11 = target intensity at (x0, y0), (x0+1, y0),
             (x0, y0+1), (x0+1, y0+1); top = (1-a) i00 + a i10, bottom = (1-a) i01 + a i11, value = (1-b) top + b bottom;
             gx = (1-b)(i10 - i00) + b (i11 - i01), gy = (1-a)(i01 - i00) + a (i11 - i10); r_I = value - I_src(pixel);
             sx = gx fx, sy = gy fy, d = (sx / q.z, sy / q.z, -((sx q.x + sy q.y) / (q.z q.z))), J_I = (q x d, d);
             w = 1 when |r_I| <= huber, else huber / |r_I|.
    terms    float64 on the widened float32 values, c = w (lambda lambda) with lambda the float32 photo weight widened:
             H[k] = J_G[i] J_G[j] + (c J_I[i]) J_I[j] for i <= j row-major (21), b[i] = J_G[i] r_G + (c J_I[i]) r_I (6),
             r_G r_G, 1 (geometric count), w (r_I r_I), 1 (photometric count): 31.  A part whose gate fails is +0.
    order    tests/mesh_register_reference.ordered_sum: chunks of 1024 pixels, 256 slots of four strided pixels, `tree`, the
             chunk sums by slot chunk % 256, `tree`.
    loop     level by level, coarse to fine, iters[l] times: sums at float32(T); stop everything when fewer than 6 pixels pass
             the photometric gate (the geometric gate is a subset of it) or H, b are not finite; x = -H^+ b through eigh without
             the directions lambda_k <= rank_tol lambda_max; T <- exp(x) T in float64; the level ends early once |w| <= 1e-6
             and |v| <= 1e-6."""
import numpy as np

from tests import mesh_register_reference as mrr

F32, F64 = np.float32, np.float64
OUT = 31
STOP = 1e-6
MIN_INLIERS = 6
RANK_TOL = 1e-9


# ---- intensity pyramid ----

def grey(color):
    c = np.ascontiguousarray(color, dtype=F32)
    out = (F32(0.299) * c[0] + F32(0.587) * c[1]) + F32(0.114) * c[2]
    assert out.dtype == F32
    return out


def half(img):
    H, W = img.shape
    h, w = H >> 1, W >> 1
    a, b = img[0:2 * h:2, 0:2 * w:2], img[0:2 * h:2, 1:2 * w:2]
    c, d = img[1:2 * h:2, 0:2 * w:2], img[1:2 * h:2, 1:2 * w:2]
    out = ((a + b) + (c + d)) * F32(0.25)
    assert out.dtype == F32
    return out


def intensity_pyramid(color, levels):
    """colour [3,H,W] -> list of [H_l,W_l] float32, coarsest first."""
    out = [grey(color)]
    for _ in range(levels - 1):
        out.append(half(out[-1]))
    return out[::-1]


# ---- per-pixel terms ----

def pixel_terms(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold, cos_threshold, photo_weight, huber):
    """-> dict of per-pixel arrays [HW]: the gates `photo`, `geo`, the float32 r_G, J_G [HW,6], r_I, J_I [HW,6], w, and u, v."""
    H, W = v_src.shape[:2]
    p = np.ascontiguousarray(v_src, dtype=F32).reshape(-1, 3)
    n = np.ascontiguousarray(n_src, dtype=F32).reshape(-1, 3)
    Is = np.ascontiguousarray(i_src, dtype=F32).reshape(-1)
    vt = np.ascontiguousarray(v_tgt, dtype=F32).reshape(-1, 3)
    nt = np.ascontiguousarray(n_tgt, dtype=F32).reshape(-1, 3)
    It = np.ascontiguousarray(i_tgt, dtype=F32).reshape(-1)
    T = np.asarray(pose, dtype=F32).reshape(4, 4)
    K = np.asarray(K, dtype=F32).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    Wm1, Hm1 = F32(W - 1), F32(H - 1)
    with np.errstate(all="ignore"):
        q = [((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)]
        u = (q[0] / q[2]) * fx + cx
        v = (q[1] / q[2]) * fy + cy
        inview = (u > 0) & (u < Wm1) & (v > 0) & (v < Hm1)
        pre = inview & (p[:, 2] > 0) & (q[2] > 0)
        us, vs = np.where(pre, u, F32(0)), np.where(pre, v, F32(0))          # nothing is converted to an integer before the test
        hw, hh = Wm1 / F32(2), Hm1 / F32(2)
        ix = (((us / hw - F32(1)) + F32(1)) / F32(2)) * Wm1
        iy = (((vs / hh - F32(1)) + F32(1)) / F32(2)) * Hm1
        ix = np.minimum(Wm1, np.maximum(ix, F32(0)))
        iy = np.minimum(Hm1, np.maximum(iy, F32(0)))
        j = np.rint(iy).astype(np.int64) * W + np.rint(ix).astype(np.int64)
        g, m = vt[j], nt[j]
        e = [q[k] - g[:, k] for k in range(3)]
        dist = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        photo = pre & (g[:, 2] > 0) & (dist <= F32(distance_threshold))
        rn = [(T[r, 0] * n[:, 0] + T[r, 1] * n[:, 1]) + T[r, 2] * n[:, 2] for r in range(3)]
        geo = photo & (((rn[0] * m[:, 0] + rn[1] * m[:, 1]) + rn[2] * m[:, 2]) > F32(cos_threshold))
        rG = (m[:, 0] * e[0] + m[:, 1] * e[1]) + m[:, 2] * e[2]

        def cross_with(d):
            return [q[1] * d[2] - q[2] * d[1], q[2] * d[0] - q[0] * d[2], q[0] * d[1] - q[1] * d[0]]

        mm = [m[:, 0], m[:, 1], m[:, 2]]
        JG = np.stack(cross_with(mm) + mm, axis=1)
        x0f, y0f = np.floor(us), np.floor(vs)
        a, b = us - x0f, vs - y0f
        x0 = np.minimum(x0f.astype(np.int64), W - 2)                          # only pixels that fail the gate are clamped
        y0 = np.minimum(y0f.astype(np.int64), H - 2)
        i00, i10, i01, i11 = It[y0 * W + x0], It[y0 * W + x0 + 1], It[(y0 + 1) * W + x0], It[(y0 + 1) * W + x0 + 1]
        one = F32(1)
        top = (one - a) * i00 + a * i10
        bot = (one - a) * i01 + a * i11
        value = (one - b) * top + b * bot
        gx = (one - b) * (i10 - i00) + b * (i11 - i01)
        gy = (one - a) * (i01 - i00) + a * (i11 - i10)
        rI = value - Is
        sx, sy = gx * fx, gy * fy
        d = [sx / q[2], sy / q[2], -((sx * q[0] + sy * q[1]) / (q[2] * q[2]))]
        JI = np.stack(cross_with(d) + d, axis=1)
        ar = np.abs(rI)
        w = np.where(ar <= F32(huber), one, F32(huber) / ar)
    for x in (u, rG, JG, rI, JI, w):
        assert x.dtype == F32
    return {"photo": photo, "geo": geo, "rG": rG, "JG": JG, "rI": rI, "JI": JI, "w": w, "u": u, "v": v}


def terms(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold, cos_threshold, photo_weight, huber):
    """-> [HW, 31] float64."""
    t = pixel_terms(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold, cos_threshold, photo_weight, huber)
    geo, photo = t["geo"], t["photo"]
    lam = F64(F32(photo_weight))
    with np.errstate(all="ignore"):
        JG, JI, rG, rI, w = (t[k].astype(F64) for k in ("JG", "JI", "rG", "rI", "w"))
        c = w * (lam * lam)
        out = np.zeros((len(rG), OUT), F64)

        def both(x, y):
            return np.where(geo, x, 0.0) + np.where(photo, y, 0.0)

        k = 0
        for i in range(6):
            for j in range(i, 6):
                out[:, k] = both(JG[:, i] * JG[:, j], (c * JI[:, i]) * JI[:, j])
                k += 1
        for i in range(6):
            out[:, 21 + i] = both(JG[:, i] * rG, (c * JI[:, i]) * rI)
        out[:, 27] = np.where(geo, rG * rG, 0.0)
        out[:, 28] = np.where(geo, 1.0, 0.0)
        out[:, 29] = np.where(photo, w * (rI * rI), 0.0)
        out[:, 30] = np.where(photo, 1.0, 0.0)
    return out


def accumulate(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold, cos_threshold, photo_weight, huber):
    """rtgs_rgbd_align_accumulate -> [31] float64."""
    with np.errstate(all="ignore"):
        return mrr.ordered_sum(terms(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold, cos_threshold,
                                     photo_weight, huber))


# ---- the loop ----

def solve(out, rank_tol=RANK_TOL):
    """-> (x, rank): x = - sum over the kept j of e_j (e_j . b) / lambda_j, added in ascending j from 0."""
    x, rank, _, _ = mrr.solve(out[:27], rank_tol)
    return x, rank


def se3_exp(x):
    """exp of the twist x = (w, v) -> 4x4 float64 (the ICP tracker's exp_se3: rotation by Rodrigues, translation J_l v)."""
    w, v = np.asarray(x[:3], dtype=F64), np.asarray(x[3:], dtype=F64)
    Wh = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    W2 = Wh @ Wh
    th = np.sqrt(np.dot(w, w))
    I = np.eye(3)
    if th <= 1e-8:
        R, Jl = I, I
    else:
        R = I + Wh * (np.sin(th) / th) + W2 * ((1.0 - np.cos(th)) / (th * th))
        Jl = I + Wh * ((1.0 - np.cos(th)) / (th * th)) + W2 * ((th - np.sin(th)) / (th * th * th))
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = Jl @ v
    return T


def level_K(K, downscale):
    Kl = np.asarray(K, dtype=F32).reshape(3, 3) * F32(downscale)
    Kl[2, 2] = F32(1)
    return Kl


def refine(init_pose, v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, downscales, iters=(3, 3, 3), distance_threshold=0.1,
           cos_threshold=0.9396926, photo_weight=0.25, huber=0.05, rank_tol=RANK_TOL, accumulate_fn=None):
    """Pyramids coarsest first, K of the full-resolution frame.  -> (T float64 [4,4], report)."""
    acc = accumulate_fn or accumulate
    T = np.array(init_pose, dtype=F64).reshape(4, 4)
    rep = {"iterations": [0] * len(downscales), "inliers_geometric": [], "inliers_photometric": [], "rank": [], "twists": [], "reason": "done"}
    first = last = None
    stop = False
    for l, ds in enumerate(downscales):
        Kl = level_K(K, ds)
        for _ in range(int(iters[l])):
            out = np.asarray(acc(v_src[l], n_src[l], i_src[l], v_tgt[l], n_tgt[l], i_tgt[l], Kl, T.astype(F32),
                                 distance_threshold, cos_threshold, photo_weight, huber), dtype=F64)
            rep["inliers_geometric"].append(int(out[28]) if np.isfinite(out[28]) else 0)
            rep["inliers_photometric"].append(int(out[30]) if np.isfinite(out[30]) else 0)
            last = out
            first = out if first is None else first
            if not out[30] >= MIN_INLIERS:
                rep["reason"], stop = "too few inliers", True
                break
            if not np.isfinite(out[:27]).all():
                rep["reason"], stop = "sums not finite", True
                break
            x, rank = solve(out, rank_tol)
            rep["rank"].append(rank)
            rep["twists"].append(x)
            T = se3_exp(x) @ T
            rep["iterations"][l] += 1
            if np.sqrt(np.dot(x[:3], x[:3])) <= STOP and np.sqrt(np.dot(x[3:], x[3:])) <= STOP:
                break
        if stop:
            break
    for name, o in (("before", first), ("after", last)):
        ok = o is not None
        rep["rms_geometric_" + name] = float(np.sqrt(o[27] / o[28])) if ok and o[28] > 0 else float("nan")
        rep["rms_photometric_" + name] = float(np.sqrt(o[29] / o[30])) if ok and o[30] > 0 else float("nan")
    return T, rep


# ---- the scenes the CPU and GPU tests share ----

WALL_Z = 2.0
WALL_XI = np.array([0.004, -0.003, 0.006, 0.020, -0.015, 0.010])             # (rotation rad, translation m)


def wall_K(H=60, W=80, f=70.0):
    return np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1]], dtype=F32)


def wall_texture(X, Y):
    """Colour [3, ...] in 0..1 of the wall point (X, Y): sinusoids of about 0.5 m period in both directions of the plane."""
    s = np.sin(2 * np.pi * X / 0.5)
    c = np.sin(2 * np.pi * Y / 0.45 + 0.7)
    d = np.sin(2 * np.pi * (X + Y) / 0.7 + 0.3)
    return np.stack([0.5 + 0.25 * s + 0.2 * c, 0.5 + 0.2 * c * s + 0.25 * d, 0.5 + 0.3 * d - 0.15 * s]).astype(F32)


def wall_view(c2w, H=60, W=80, f=70.0, textured=True, normal=(0.0, 0.0, -1.0)):
    """The plane Z = WALL_Z of the world seen by the camera `c2w` (4x4): -> (depth [H,W] float32, colour [3,H,W] float32,
    vertex [H,W,3] float32, normal [H,W,3] float32 = the plane's normal in the camera, analytic)."""
    K = wall_K(H, W, f).astype(F64)
    c2w = np.asarray(c2w, dtype=F64)
    xs, ys = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64))
    rays = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], axis=-1)
    rw = rays @ c2w[:3, :3].T
    depth = (WALL_Z - c2w[2, 3]) / rw[..., 2]
    world = rw * depth[..., None] + c2w[:3, 3]
    colour = wall_texture(world[..., 0], world[..., 1]) if textured else np.full((3, H, W), 0.5, F32)
    depth = depth.astype(F32)
    K32 = wall_K(H, W, f)
    vertex = np.stack([(xs.astype(F32) - K32[0, 2]) / K32[0, 0], (ys.astype(F32) - K32[1, 2]) / K32[1, 1],
                       np.ones((H, W), F32)], axis=-1) * depth[..., None]
    nrm = np.broadcast_to((c2w[:3, :3].T @ np.asarray(normal, dtype=F64)).astype(F32), (H, W, 3)).copy()
    return depth, colour, vertex.astype(F32), nrm


def wall_pair(H=60, W=80, textured=True, xi=WALL_XI):
    """Target = the camera at the world's origin looking down +Z at the wall; source = the camera exp(xi).  The true
    source -> target pose is exp(xi).  -> dict with v_src n_src i_src v_tgt n_tgt i_tgt (single level), K, truth."""
    truth = se3_exp(xi)
    _, c_t, v_t, n_t = wall_view(np.eye(4), H, W, textured=textured)
    _, c_s, v_s, n_s = wall_view(truth, H, W, textured=textured)
    return {"v_src": v_s, "n_src": n_s, "i_src": grey(c_s), "v_tgt": v_t, "n_tgt": n_t, "i_tgt": grey(c_t),
            "K": wall_K(H, W), "truth": truth}
