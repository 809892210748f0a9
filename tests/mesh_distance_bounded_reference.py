"""Plain-numpy definition of the BOUNDED point-to-mesh query (include/rtgs_slam.h, rtgs_mesh_distance_query_bounded;
mesh_ops.MeshDistance.query(max_distance=...)): "the nearest face within D, or nothing".  It is the brute force of
tests/mesh_distance_reference.py with the rows beyond the bound blanked, so the kernel's early stop must not show in any bit.
Used only by tests.

    max_d2_of(D)        m = float32(D), max_d2 = m m rounded to float32: the expression register_to_mesh gates with.
    nearest_within      (d2*, f*) = nearest(...); row i is (d2*[i], f*[i]) when d2*[i] <= max_d2 (float32; equality keeps the
                        row, a NaN drops it) and (inf, -1) otherwise - so also for a point with a non-finite coordinate.
                        max_d2 = inf is nearest itself, max_d2 = 0 keeps only exact zeros.
    eval_mesh_surface_truncated   the composition evaluation.eval_mesh_surface(max_distance=D) is held to: a distance beyond D
                        counts as D (its d2 is replaced by max_d2), the normal consistency runs over the rows within the bound."""
import numpy as np

from tests.mesh_distance_reference import F32, hit_normals, nearest, normal_consistency


def max_d2_of(max_distance):
    m = F32(max_distance)
    with np.errstate(over="ignore"):
        out = m * m
    assert out.dtype == F32
    return out


def nearest_within(points, vertices, faces, max_d2):
    """-> (d2 float32 [N], face int32 [N]); max_d2 a float32, >= 0."""
    max_d2 = F32(max_d2)
    assert max_d2 >= 0
    d2, face = nearest(points, vertices, faces)
    keep = d2 <= max_d2                                               # False for a NaN, and for the inf of a non-finite point ...
    keep &= face >= 0                                                 # ... also when max_d2 is inf
    return np.where(keep, d2, F32(np.inf)).astype(F32), np.where(keep, face, -1).astype(np.int32)


def eval_mesh_surface_truncated(rec_samples, rec_own_face, rec_v, rec_f, gt_samples, gt_own_face, gt_v, gt_f, dist_thres=(0.03,),
                                max_distance=0.05):
    """tests/mesh_distance_reference.eval_mesh_surface with both directions queried through nearest_within(max_d2_of(D)): the
    same keys, and max_distance, beyond_acc, beyond_comp - the rows beyond the bound."""
    assert max_distance > max(dist_thres)
    max_d2 = max_d2_of(max_distance)
    res = {}
    sides = (("acc", rec_samples, rec_own_face, rec_v, rec_f, gt_v, gt_f), ("comp", gt_samples, gt_own_face, gt_v, gt_f, rec_v, rec_f))
    frac = {}
    for name, pts, own, ov, of, tv, tf in sides:
        d2, face = nearest_within(pts, tv, tf, max_d2)
        beyond = face < 0
        d = np.sqrt(np.where(beyond, max_d2, d2).astype(np.float64))   # the float32 d2, its root in float64
        n = len(d)
        res["accuracy" if name == "acc" else "completion"] = float(d.sum()) / n * 100.0
        frac[name] = [float((d < t).sum()) / n * 100.0 for t in dist_thres]
        s, cnt = normal_consistency(hit_normals(ov, of, own), hit_normals(tv, tf, face))
        res["normal_consistency_" + name] = s / cnt if cnt else float("nan")
        res["normal_samples_" + name] = cnt
        res["beyond_" + name] = int(beyond.sum())
    for j, t in enumerate(dist_thres):
        P, R = frac["acc"][j], frac["comp"][j]
        res[f"P (< {t})"], res[f"R (< {t})"] = P, R
        res[f"F1 (< {t})"] = 2 * P * R / (P + R) if P + R > 0 else float("nan")
    res["normal_consistency"] = 0.5 * (res["normal_consistency_acc"] + res["normal_consistency_comp"])
    res["max_distance"] = float(max_distance)
    return res
