"""The definition of rtgs_rigid_ransac (csrc/rigid_ransac.hip, keypoints.rigid_ransac_pairs) in numpy float64: the match filter
and the 3-D - 3-D rigid RANSAC of one keyframe pair, written with + - * / and sqrt alone in a stated order, so that the kernel
matches it bit for bit.  It is a definition of its own: keypoints.ransac_rigid solves the same least-squares problems by LAPACK's
SVD, which cannot be restated on a device, and stays what it is.

THE WAVE ORDER of a sum over a flat list v[0 .. n - 1] is tests/place_reference.wave_sum: lane l of 64 adds v[l], v[l + 64], ..
in that order onto +0.0, then the tree t[:o] = t[:o] + t[o:2 o], o = 32, 16, .. 1.  A gated-out element counts as +0.0.  For a
list of three that is ((0.0 + v0) + (0.0 + v2)) + (0.0 + v1).

FILTER (keypoints.filter_matches' rule).  m_ba [nb][3]: b's keypoints against a's (index, distance, second), m_ab [na][3] the
other way.  Row i of m_ba survives when 0 <= j < na, m_ab[j][0] == i, d <= max_hamming and float64(d) <= ratio * float64(second).
The survivors in order of i, the first CAP = 1024 of them (two float64 point sets of 1024 are 48 KiB of LDS), are the n matches:
A[k] = xyz_a[j], B[k] = xyz_b[i].  `survivors` counts them before the cap.

HYPOTHESIS h = 0 .. iters - 1 (iters <= 65535), n >= 3: the indices mix32(seed + 3 h + j) mod n, j = 0, 1, 2, in uint32.  It is
skipped when two indices are equal or when, in either frame, with e1 = p1 - p0, e2 = p2 - p0, s = (ex ex + ey ey) + ez ez,
c = e1 x e2 = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x):
    not s1 > 1e-18, or not s2 > 1e-18, or not (cx cx + cy cy) + cz cz >= 0.01 * (s1 * s2).
Its pose is FIT of the list (p0, p1, p2), nothing gated out.

FIT of a list of pairs (A_i, B_i) with a gate, k gated in (Horn's closed form; R, t with A ~ R B + t):
    ca = wave_sum(A) / k, cb = wave_sum(B) / k                       per coordinate; k as float64
    S[r][c] = wave_sum((B_i[r] - cb[r]) * (A_i[c] - ca[c]))          nine sums; x, y, z = 0, 1, 2
    N00 = (Sxx + Syy) + Szz   N11 = (Sxx - Syy) - Szz   N22 = (Syy - Sxx) - Szz   N33 = (Szz - Sxx) - Syy
    N01 = Syz - Szy   N02 = Szx - Sxz   N03 = Sxy - Syx   N12 = Sxy + Syx   N13 = Szx + Sxz   N23 = Syz + Szy
    SWEEPS = 8 cyclic Jacobi sweeps over (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), V = I at the start.  A rotation with
    apq == 0 is skipped, otherwise
        theta = (aqq - app) / (2.0 * apq);  t = (theta >= 0 ? 1.0 : -1.0) / (|theta| + sqrt(theta * theta + 1.0))
        c = 1.0 / sqrt(t * t + 1.0);  s = t * c
        app' = app - t * apq;  aqq' = aqq + t * apq;  apq' = 0
        arp' = c * arp - s * arq;  arq' = s * arp + c * arq          for the two r outside (p, q), kept symmetric
        vrp' = c * vrp - s * vrq;  vrq' = s * vrp + c * vrq          for r = 0 .. 3
    m = the index of the largest diagonal entry, the lowest on a tie; (w, x, y, z) = V[:, m] / sqrt(((w w + x x) + y y) + z z)
    R = [[1 - 2 (yy + zz), 2 (xy - wz), 2 (xz + wy)], [2 (xy + wz), 1 - 2 (xx + zz), 2 (yz - wx)], [2 (xz - wy), 2 (yz + wx), 1 - 2 (xx + yy)]]
    t[r] = ca[r] - ((R[r][0] * cb[0] + R[r][1] * cb[1]) + R[r][2] * cb[2])

COUNT.  d[r] = (((R[r][0] * Bx + R[r][1] * By) + R[r][2] * Bz) + t[r]) - A[r];  d2 = (dx dx + dy dy) + dz dz; a match is an
inlier when d2 <= inlier_dist * inlier_dist.  The hypothesis with the highest count wins, the earliest h on a tie.

REFIT, up to three rounds from the winner's pose and inliers: stop when fewer than 3 inliers; FIT of all n matches gated by the
inliers; COUNT; stop without taking the round when it has fewer inliers; take it; stop when the inlier set did not change.

OUT: T = [R t; 0 0 0 1], n, the inlier count, rms = sqrt(wave_sum(d2 gated by the inliers) / count) (0 without an inlier), the
winning h, the inlier flags and the (i, j) of the n matches.  Without a valid hypothesis (and for n < 3): h = -1, no inlier,
T and rms zero."""
import numpy as np

from tests.keypoint_reference import mix32
from tests.place_reference import wave_sum

F64 = np.float64
CAP = 1024
SWEEPS = 8
MAX_ITERS = 65535
PQ = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def filter_matches(m_ba, m_ab, max_hamming=64, ratio=0.8):
    """-> ([(i, j)] of the n matches, survivors before the cap)."""
    m_ba, m_ab = np.asarray(m_ba).reshape(-1, 3), np.asarray(m_ab).reshape(-1, 3)
    out = []
    for i, (j, d, second) in enumerate(m_ba.tolist()):
        if 0 <= j < len(m_ab) and int(m_ab[j][0]) == i and d <= int(max_hamming) and F64(d) <= F64(ratio) * F64(second):
            out.append((i, int(j)))
    return out[:CAP], len(out)


def fit(A, B, gate=None):
    """A, B [..., k, 3] float64, gate [..., k] bool (default: all) -> R [..., 3, 3], t [..., 3]."""
    A, B = np.asarray(A, dtype=F64), np.asarray(B, dtype=F64)
    gate = np.ones(A.shape[:-1], dtype=bool) if gate is None else np.asarray(gate, dtype=bool)
    k = gate.sum(axis=-1).astype(F64)
    g = lambda v: wave_sum(np.where(gate, v, F64(0.0)))
    with np.errstate(all="ignore"):
        ca = [g(A[..., c]) / k for c in range(3)]
        cb = [g(B[..., c]) / k for c in range(3)]
        S = [[g((B[..., r] - cb[r][..., None]) * (A[..., c] - ca[c][..., None])) for c in range(3)] for r in range(3)]
        (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
        a = {(0, 0): (Sxx + Syy) + Szz, (1, 1): (Sxx - Syy) - Szz, (2, 2): (Syy - Sxx) - Szz, (3, 3): (Szz - Sxx) - Syy,
             (0, 1): Syz - Szy, (0, 2): Szx - Sxz, (0, 3): Sxy - Syx, (1, 2): Sxy + Syx, (1, 3): Szx + Sxz, (2, 3): Syz + Szy}
        key = lambda r, c: (r, c) if r <= c else (c, r)
        one, zero = np.ones_like(k), np.zeros_like(k)
        v = [[one if r == c else zero for c in range(4)] for r in range(4)]
        for _ in range(SWEEPS):
            for p, q in PQ:
                app, aqq, apq = a[(p, p)], a[(q, q)], a[(p, q)]
                on = apq != 0.0
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta >= 0, F64(1.0), F64(-1.0)) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                a[(p, p)] = np.where(on, app - t * apq, app)
                a[(q, q)] = np.where(on, aqq + t * apq, aqq)
                a[(p, q)] = np.where(on, F64(0.0), apq)
                for r in range(4):
                    if r not in (p, q):
                        arp, arq = a[key(r, p)], a[key(r, q)]
                        a[key(r, p)] = np.where(on, c * arp - s * arq, arp)
                        a[key(r, q)] = np.where(on, s * arp + c * arq, arq)
                for r in range(4):
                    vrp, vrq = v[r][p], v[r][q]
                    v[r][p] = np.where(on, c * vrp - s * vrq, vrp)
                    v[r][q] = np.where(on, s * vrp + c * vrq, vrq)
        best, quat = a[(0, 0)], [v[r][0] for r in range(4)]
        for m in range(1, 4):
            win = a[(m, m)] > best
            best = np.where(win, a[(m, m)], best)
            quat = [np.where(win, v[r][m], quat[r]) for r in range(4)]
        w, x, y, z = quat
        norm = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / norm, x / norm, y / norm, z / norm
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        R = [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
             [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
             [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]
        t = [ca[r] - ((R[r][0] * cb[0] + R[r][1] * cb[1]) + R[r][2] * cb[2]) for r in range(3)]
    return np.stack([np.stack(row, axis=-1) for row in R], axis=-2), np.stack(t, axis=-1)


def residual2(R, t, A, B):
    """R [..., 3, 3], t [..., 3], A, B [n, 3] -> d2 [..., n]."""
    with np.errstate(all="ignore"):
        d = [(((R[..., r, 0, None] * B[:, 0] + R[..., r, 1, None] * B[:, 1]) + R[..., r, 2, None] * B[:, 2]) + t[..., r, None]) - A[:, r]
             for r in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def spread(p):
    """p [..., 3, 3]: the triplets' points -> bool [...]."""
    e1, e2 = p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :]
    sq = lambda e: (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    s1, s2 = sq(e1), sq(e2)
    c = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                  e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], axis=-1)
    return (s1 > 1e-18) & (s2 > 1e-18) & (sq(c) >= 0.01 * (s1 * s2))


def triplets(n, iters, seed):
    """-> int64 [iters, 3]."""
    return np.array([[mix32((int(seed) + 3 * h + j) & 0xFFFFFFFF) % n for j in range(3)] for h in range(int(iters))], dtype=np.int64).reshape(-1, 3)


def ransac(A, B, iters=512, inlier_dist=0.05, seed=0):
    """The n matches' points A (in a's camera), B (in b's) [n, 3] -> {"T" [4, 4], "inliers", "rms", "h", "mask" bool [n]}."""
    A, B = np.asarray(A, dtype=F64).reshape(-1, 3), np.asarray(B, dtype=F64).reshape(-1, 3)
    n = A.shape[0]
    if not 1 <= int(iters) <= MAX_ITERS or n > CAP or B.shape[0] != n:
        raise ValueError("ransac: 1 <= iters <= 65535, at most CAP matches, as many points in a as in b")
    none = {"T": np.zeros((4, 4)), "inliers": 0, "rms": 0.0, "h": -1, "mask": np.zeros(n, dtype=bool)}
    if n < 3:
        return none
    lim = F64(inlier_dist) * F64(inlier_dist)
    idx = triplets(n, iters, seed)
    ok = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    ok &= spread(A[idx]) & spread(B[idx])
    hs = np.nonzero(ok)[0]
    if len(hs) == 0:
        return none
    R, t = fit(A[idx[hs]], B[idx[hs]])
    counts = (residual2(R, t, A, B) <= lim).sum(axis=1)
    w = int(np.argmax(counts))                                        # the first of equal maxima: the earliest h
    R, t, h = R[w], t[w], int(hs[w])
    mask = residual2(R, t, A, B) <= lim
    for _ in range(3):
        if mask.sum() < 3:
            break
        R2, t2 = fit(A, B, mask)
        m2 = residual2(R2, t2, A, B) <= lim
        if m2.sum() < mask.sum():
            break
        same = np.array_equal(m2, mask)
        R, t, mask = R2, t2, m2
        if same:
            break
    T = np.zeros((4, 4))
    T[:3, :3], T[:3, 3], T[3, 3] = R, t, 1.0
    cnt = int(mask.sum())
    rms = float(np.sqrt(wave_sum(np.where(mask, residual2(R, t, A, B), F64(0.0))) / F64(cnt))) if cnt else 0.0
    return {"T": T, "inliers": cnt, "rms": rms, "h": h, "mask": mask}


def pair(m_ba, m_ab, xyz_a, xyz_b, max_hamming=64, ratio=0.8, iters=512, inlier_dist=0.05, seed=0):
    """One keyframe pair -> ransac's dict plus "n", "survivors", "ij" int32 [n, 2]."""
    ij, survivors = filter_matches(m_ba, m_ab, max_hamming, ratio)
    xa, xb = np.asarray(xyz_a, dtype=F64).reshape(-1, 3), np.asarray(xyz_b, dtype=F64).reshape(-1, 3)
    out = ransac(xa[[j for _, j in ij]], xb[[i for i, _ in ij]], iters, inlier_dist, seed)
    out.update(n=len(ij), survivors=survivors, ij=np.asarray(ij, dtype=np.int32).reshape(-1, 2))
    return out
