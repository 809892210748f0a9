"""Plain-numpy restatement of the RGB-D pose refinement with exposure compensation (include/rtgs_icp.h, "RGB-D refinement";
csrc/rgbd_exposure.hip; rtg_slam_amd/rgbd_align.py): a gain `alpha` and an offset `beta` that take the source (current) frame's
intensity into the target's exposure are unknowns 7 and 8 of the normal equations of tests/rgbd_align_reference.py, and the
target may be a composite of the map's rendered colour and the frame's own.  Used only by tests; it is the definition the kernels
and the host loop are held to, bit for bit.  Everything not restated here is rgbd_align_reference's, imported and unchanged.

    pixel    rgbd_align_reference.pixel_terms called with the TRANSFORMED source intensity: with float32 alpha, beta,
             Ic = alpha I_src (rounded), Ic = Ic + beta (rounded), so r_I = value - Ic and the Huber weight is taken on that
             r_I; gates, q, u, v, the nearest target pixel, r_G, J_G, value, gx, gy and J_I do not see the intensity and are the
             same.  J8 = (J_I[0..5], -I_src, -1) with the RAW I_src: the derivative of r_I by (twist, alpha, beta).
             The exposure maps source into target - not the other way - because the target is what stays: in model mode it is
             the map's colour, whose exposure is one for the whole sequence, and every frame is brought to it.
    terms    float64 on the widened float32 values, c = w (lambda lambda):
             H[k] = (geo and i < 6 and j < 6 ? J_G[i] J_G[j] : +0) + (c J8[i]) J8[j] for i <= j < 8 row-major (36),
             b[i] = (geo and i < 6 ? J_G[i] r_G : +0) + (c J8[i]) r_I (8), then r_G r_G, 1 (geometric count), w (r_I r_I),
             1 (photometric count) at 44..47: 48.  A pixel whose photometric gate fails contributes +0.
    order    tests/mesh_register_reference.ordered_sum, unchanged.
    solve    eigh of the 8 x 8 matrix; the directions lambda_k <= rank_tol lambda_max are dropped;
             x = - sum e_j (e_j . b) / lambda_j in ascending j.
    loop     rgbd_align_reference.refine's with the state (T, alpha, beta) in float64: T <- exp(x[:6]) T, alpha += x[6],
             beta += x[7]; the sums are taken at float32(T), float32(alpha), float32(beta).  A level ends early once |w|, |v|,
             |x[6]|, |x[7]| are all <= 1e-6.  An update that would take alpha outside [0.25, 4] or |beta| above 0.5 is not
             applied: the loop stops with the reason "exposure out of range", keeps the pose from before that update and
             returns the exposure (1, 0).
    target   composite: per pixel of the full-resolution frame, replaced = (depth_filled != depth_rendered) in float32 (the
             model's rendered depth before and after fill_model_depth: where they differ the tracker's target geometry is
             the frame's, so its colour must be too); a replaced pixel takes alpha grey(frame colour) + beta in two rounded
             float32 steps - the frame's colour in the MAP's exposure, or the next frame would be pulled towards this frame's
             exposure over those pixels; every other pixel takes grey(render colour).  Then the 2 x 2 means of `half`."""
import numpy as np

from tests import mesh_register_reference as mrr
from tests import rgbd_align_reference as rar

F32, F64 = np.float32, np.float64
OUT = 48
NU = 8
NH = NU * (NU + 1) // 2
STOP = rar.STOP
MIN_INLIERS = rar.MIN_INLIERS
RANK_TOL = rar.RANK_TOL
ALPHA_MIN, ALPHA_MAX, BETA_MAX = 0.25, 4.0, 0.5


def to_target_exposure(intensity, alpha, beta):
    """alpha I + beta in two rounded float32 steps."""
    I = np.ascontiguousarray(intensity, dtype=F32)
    with np.errstate(all="ignore"):
        out = F32(alpha) * I
        out = out + F32(beta)
    assert out.dtype == F32
    return out


# ---- per-pixel terms ----

def pixel_terms(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold, cos_threshold, photo_weight, huber,
                alpha, beta):
    """rgbd_align_reference.pixel_terms with the transformed source intensity, plus "J8" [HW,8] float32."""
    t = rar.pixel_terms(v_src, n_src, to_target_exposure(i_src, alpha, beta), v_tgt, n_tgt, i_tgt, K, pose, distance_threshold,
                        cos_threshold, photo_weight, huber)
    Is = np.ascontiguousarray(i_src, dtype=F32).reshape(-1)
    t["J8"] = np.concatenate([t["JI"], -Is[:, None], np.full((len(Is), 1), -1, F32)], axis=1)
    assert t["J8"].dtype == F32
    return t


def terms(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold, cos_threshold, photo_weight, huber, alpha, beta):
    """-> [HW, 48] float64."""
    t = pixel_terms(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold, cos_threshold, photo_weight, huber,
                    alpha, beta)
    geo, photo = t["geo"], t["photo"]
    lam = F64(F32(photo_weight))
    with np.errstate(all="ignore"):
        JG, J8, rG, rI, w = (t[k].astype(F64) for k in ("JG", "J8", "rG", "rI", "w"))
        c = w * (lam * lam)
        out = np.zeros((len(rG), OUT), F64)
        zero = np.zeros(len(rG), F64)
        k = 0
        for i in range(NU):
            for j in range(i, NU):
                g = np.where(geo, JG[:, i] * JG[:, j], 0.0) if j < 6 else zero
                out[:, k] = g + np.where(photo, (c * J8[:, i]) * J8[:, j], 0.0)
                k += 1
        for i in range(NU):
            g = np.where(geo, JG[:, i] * rG, 0.0) if i < 6 else zero
            out[:, NH + i] = g + np.where(photo, (c * J8[:, i]) * rI, 0.0)
        out[:, 44] = np.where(geo, rG * rG, 0.0)
        out[:, 45] = np.where(geo, 1.0, 0.0)
        out[:, 46] = np.where(photo, w * (rI * rI), 0.0)
        out[:, 47] = np.where(photo, 1.0, 0.0)
    return out


def accumulate(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold, cos_threshold, photo_weight, huber,
               alpha, beta):
    """rtgs_rgbd_align_accumulate_exposure -> [48] float64."""
    with np.errstate(all="ignore"):
        return mrr.ordered_sum(terms(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold, cos_threshold,
                                     photo_weight, huber, alpha, beta))


def pose_block(out):
    """The 48 sums -> the 31 of rtgs_rgbd_align_accumulate: the 21 + 6 entries of the pose block and the four statistics."""
    idx, k = [], 0
    for i in range(NU):
        for j in range(i, NU):
            if j < 6:
                idx.append(k)
            k += 1
    return np.concatenate([np.asarray(out)[idx], np.asarray(out)[NH:NH + 6], np.asarray(out)[44:48]])


# ---- the loop ----

def solve8(out, rank_tol=RANK_TOL):
    """-> (x [8], rank): x = - sum over the kept j of e_j (e_j . b) / lambda_j, added in ascending j from 0."""
    A = np.zeros((NU, NU), F64)
    k = 0
    for i in range(NU):
        for j in range(i, NU):
            A[i, j] = A[j, i] = out[k]
            k += 1
    b = np.array(out[NH:NH + NU], dtype=F64)
    lam, E = np.linalg.eigh(A)
    x, rank = np.zeros(NU, F64), 0
    for j in range(NU):
        if lam[j] > rank_tol * lam[NU - 1]:
            x = x - E[:, j] * (np.dot(E[:, j], b) / lam[j])
            rank += 1
    return x, rank


def in_range(alpha, beta):
    return bool(ALPHA_MIN <= alpha <= ALPHA_MAX and abs(beta) <= BETA_MAX)


def refine(init_pose, v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, downscales, iters=(3, 3, 3), distance_threshold=0.1,
           cos_threshold=0.9396926, photo_weight=0.25, huber=0.05, rank_tol=RANK_TOL, exposure=(1.0, 0.0), accumulate_fn=None):
    """Pyramids coarsest first, K of the full-resolution frame.  -> (T float64 [4,4], report); the report is
    rgbd_align_reference.refine's plus "exposure" (the final alpha, beta) and "exposure_steps" (after every update)."""
    acc = accumulate_fn or accumulate
    T = np.array(init_pose, dtype=F64).reshape(4, 4)
    alpha, beta = F64(exposure[0]), F64(exposure[1])
    rep = {"iterations": [0] * len(downscales), "inliers_geometric": [], "inliers_photometric": [], "rank": [], "twists": [],
           "exposure_steps": [], "reason": "done"}
    first = last = None
    stop = False
    for l, ds in enumerate(downscales):
        Kl = rar.level_K(K, ds)
        for _ in range(int(iters[l])):
            out = np.asarray(acc(v_src[l], n_src[l], i_src[l], v_tgt[l], n_tgt[l], i_tgt[l], Kl, T.astype(F32),
                                 distance_threshold, cos_threshold, photo_weight, huber, F32(alpha), F32(beta)), dtype=F64)
            rep["inliers_geometric"].append(int(out[45]) if np.isfinite(out[45]) else 0)
            rep["inliers_photometric"].append(int(out[47]) if np.isfinite(out[47]) else 0)
            last = out
            first = out if first is None else first
            if not out[47] >= MIN_INLIERS:
                rep["reason"], stop = "too few inliers", True
                break
            if not np.isfinite(out[:NH + NU]).all():
                rep["reason"], stop = "sums not finite", True
                break
            x, rank = solve8(out, rank_tol)
            rep["rank"].append(rank)
            rep["twists"].append(x)
            if not in_range(alpha + x[6], beta + x[7]):
                rep["reason"], stop = "exposure out of range", True
                alpha, beta = F64(1.0), F64(0.0)
                break
            T = rar.se3_exp(x[:6]) @ T
            alpha, beta = alpha + x[6], beta + x[7]
            rep["exposure_steps"].append((float(alpha), float(beta)))
            rep["iterations"][l] += 1
            if (np.sqrt(np.dot(x[:3], x[:3])) <= STOP and np.sqrt(np.dot(x[3:6], x[3:6])) <= STOP and abs(x[6]) <= STOP
                    and abs(x[7]) <= STOP):
                break
        if stop:
            break
    for name, o in (("before", first), ("after", last)):
        ok = o is not None
        rep["rms_geometric_" + name] = float(np.sqrt(o[44] / o[45])) if ok and o[45] > 0 else float("nan")
        rep["rms_photometric_" + name] = float(np.sqrt(o[46] / o[47])) if ok and o[47] > 0 else float("nan")
    rep["exposure"] = (float(alpha), float(beta))
    return T, rep


# ---- the composite target ----

def composite(render_color, frame_color, depth_rendered, depth_filled, alpha, beta):
    """colours [3,H,W], depths [H,W] -> [H,W] float32."""
    H, W = np.asarray(render_color).shape[1:]
    dr = np.ascontiguousarray(depth_rendered, dtype=F32).reshape(H, W)
    df = np.ascontiguousarray(depth_filled, dtype=F32).reshape(H, W)
    replaced = df != dr
    out = np.where(replaced, to_target_exposure(rar.grey(frame_color), alpha, beta), rar.grey(render_color))
    assert out.dtype == F32
    return out


def target_intensity_pyramid(render_color, frame_color, depth_rendered, depth_filled, alpha, beta, levels):
    """rtgs_rgbd_target_intensity -> list of [H_l,W_l] float32, coarsest first."""
    out = [composite(render_color, frame_color, depth_rendered, depth_filled, alpha, beta)]
    for _ in range(levels - 1):
        out.append(rar.half(out[-1]))
    return out[::-1]


# ---- the scenes the CPU and GPU tests share ----

EXPOSURE_CASES = ((1.0, 0.0), (1.25, -0.06), (0.8, 0.08))          # (gain, offset) of the source frame's intensity


def exposed_wall_pair(H=60, W=80, gain=1.0, offset=0.0, textured=True):
    """rgbd_align_reference.wall_pair with the source frame's intensity at `gain`, `offset`: the exposure that undoes it is
    alpha = 1 / gain, beta = -offset / gain."""
    s = rar.wall_pair(H, W, textured=textured)
    s["i_src"] = to_target_exposure(s["i_src"], gain, offset)
    return s
