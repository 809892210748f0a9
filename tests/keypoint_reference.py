"""The definition of the keypoint registration of wide-baseline revisits (csrc/keypoints.hip, rtg_slam_amd/keypoints.py) in numpy.
Everything after the grey value is integer arithmetic: the kernels match this file bit for bit.

GREY IMAGE.  g8 = clamp(floor(grey 255 + 0.5), 0, 255) as uint8; grey is the float32 chain (0.299 r + 0.587 g) + 0.114 b of
rgbd_align_reference.grey, times 255 and plus 0.5 in float32, not contracted.  A NaN counts as 0.  box5[y, x] is the sum of g8
over the 5 x 5 pixels around (x, y), pixels outside the image counting as 0 (int32).

CORNER SCORE (FAST-9).  CIRCLE lists the 16 pixels (dx, dy) of the circle of radius 3, clockwise from (0, -3).  With c[k] the g8
there and p the centre's,  score = max( max_s min_{k<9} (c[s + k] - p), max_s min_{k<9} (p - c[s + k]) ),  indices mod 16: the
largest threshold at which p is still a FAST-9 corner (negative where it is none at any).  Pixels nearer than 3 to the border
have no score.

ELIGIBLE.  score > threshold, 16 <= x < W - 16, 16 <= y < H - 16, depth finite and > 0.  Every other pixel, and every pixel
outside the image, counts as score 0 from here on.

3 x 3 NON-MAXIMUM SUPPRESSION.  A pixel of score > 0 survives when its score is strictly greater than that of each of the four
neighbours that come earlier in raster order (the three above, the one to the left) and at least that of each of the four later.

ONE KEYPOINT PER CELL.  Cells of c x c pixels anchored at (0, 0), ceil(W / c) x ceil(H / c) of them, row by row, partial ones at
the right and bottom included.  A cell keeps its survivor of the highest score, on a tie the one with the lowest row-major pixel
index.  slots [cells, 4] int32 = x, y, score, bin; an empty slot is 0, 0, 0, -1.  The keypoints are the non-empty slots in order.

ORIENTATION.  m10 = sum dx g8, m01 = sum dy g8 over the disc dx^2 + dy^2 <= 169.  bin = argmax_k (C_k m10 + S_k m01), k = 0 .. 31,
(C_k, S_k) = rint(16384 (cos, sin)(2 pi k / 32)) (direction_table), in int64, ties to the lowest k.  Not oriented: bin 0.

DESCRIPTOR.  256 bits in 8 uint32, bit i in word i / 32 at position i % 32: box5(P1_i) < box5(P2_i) at the keypoint plus the
pattern's points (rtg_slam_amd/keypoint_pattern.PATTERN: x1, y1, x2, y2) turned into the keypoint's bin: for bin k the point (x, y)
becomes (rint(c x - s y), rint(s x + c y)), (c, s) = (cos, sin)(2 pi k / 32) in float64 (rotated_patterns, [32, 256, 4] int8).
A point of the disc turned and rounded keeps |x|, |y| <= 13, so with box5's two pixels every read stays inside the 16-pixel margin.

MATCH of a query set against a reference set (match): per query the reference index of the least Hamming distance (ties to the
lowest index), that distance, and the least distance over all other reference indices, 257 when there is none; an empty
reference set gives -1, 257, 257.

FILTER (filter_matches).  (i in b, j in a) is a match when i's best in a is j and j's best in b is i, d <= max_hamming and
d <= ratio second, second taken on b's side (float64 product).  In order of i.

RIGID POSE (ransac_rigid).  Hypothesis h = 0 .. iters - 1 draws the match indices  mix32(seed + 3 h + j) mod n,  j = 0, 1, 2
(mix32 below: a counter-based 32-bit integer hash, no state).  A triplet is skipped when two of its indices are equal or when,
in either frame, with e1 = p1 - p0 and e2 = p2 - p0, |e1| or |e2| <= 1e-9 or |e1 x e2| < 0.1 |e1| |e2| (the angle at p0 is
below 5.74 or above 174.26 degrees).  Kabsch (SVD, det-corrected) on the three pairs gives (R, t) with p_a = R p_b + t; the
inliers are the matches with |R p_b + t - p_a| <= inlier_dist; the highest count wins, the earliest on a tie.  Then up to three
rounds: refit on the inliers, recount; a round that loses inliers is dropped and ends the rounds, one that leaves the set
unchanged ends them too.  -> (T 4 x 4 float64 = T_a^-1 T_b, inlier mask, rms of the inliers' residuals) or None with fewer
than 3 matches or no valid triplet."""
import numpy as np

from rtg_slam_amd.keypoint_pattern import PATTERN
from tests.rgbd_align_reference import grey

F32 = np.float32
MARGIN, RADIUS, BINS, NO_MATCH = 16, 13, 32, 257
CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
          (-2, -2), (-1, -3))


def grey8(color):
    v = np.floor(grey(color) * F32(255.0) + F32(0.5))
    assert v.dtype == F32
    v = np.where(v >= 0, v, F32(0.0))                               # NaN -> 0
    return np.where(v > 255, F32(255.0), v).astype(np.uint8)


def box5(g8):
    H, W = g8.shape
    pad = np.zeros((H + 4, W + 4), dtype=np.int32)
    pad[2:-2, 2:-2] = g8
    return sum(pad[dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)).astype(np.int32)


def fast_score(g8):
    """[H, W] int32; 0 nearer than 3 to the border."""
    H, W = g8.shape
    out = np.zeros((H, W), dtype=np.int32)
    if H < 7 or W < 7:
        return out
    g = g8.astype(np.int32)
    p = g[3:H - 3, 3:W - 3]
    d = np.stack([g[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - p for dx, dy in CIRCLE])
    bright = np.max([np.min([d[(s + k) % 16] for k in range(9)], axis=0) for s in range(16)], axis=0)
    dark = np.max([np.min([-d[(s + k) % 16] for k in range(9)], axis=0) for s in range(16)], axis=0)
    out[3:H - 3, 3:W - 3] = np.maximum(bright, dark)
    return out


def eligible_score(g8, depth, threshold):
    H, W = g8.shape
    z = np.asarray(depth, dtype=F32).reshape(H, W)
    s = fast_score(g8)
    ok = (s > int(threshold)) & np.isfinite(z) & (z > 0)
    inside = np.zeros((H, W), dtype=bool)
    inside[MARGIN:H - MARGIN, MARGIN:W - MARGIN] = True
    return np.where(ok & inside, s, 0).astype(np.int32)


def nms(score):
    H, W = score.shape
    pad = np.zeros((H + 2, W + 2), dtype=np.int32)
    pad[1:-1, 1:-1] = score
    at = lambda dy, dx: pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    keep = score > 0
    for dy, dx in ((-1, -1), (-1, 0), (-1, 1), (0, -1)):
        keep &= score > at(dy, dx)
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        keep &= score >= at(dy, dx)
    return keep


def cell_slots(score, keep, cell):
    """-> [cells, 4] int32: x, y, score, bin (-1: detect does not set it)."""
    H, W = score.shape
    c = int(cell)
    ncx, ncy = -(-W // c), -(-H // c)
    slots = np.zeros((ncx * ncy, 4), dtype=np.int32)
    slots[:, 3] = -1
    live = np.where(keep, score, 0)
    for cy in range(ncy):
        for cx in range(ncx):
            blk = live[cy * c:(cy + 1) * c, cx * c:(cx + 1) * c]
            if blk.max() > 0:
                i = int(np.argmax(blk))                              # the first of equal maxima in the cell's row-major order
                slots[cy * ncx + cx, :3] = (cx * c + i % blk.shape[1], cy * c + i // blk.shape[1], blk.reshape(-1)[i])
    return slots


def detect(color, depth, threshold=20, cell=16):
    """-> g8 [H, W] uint8, box5 [H, W] int32, slots [cells, 4] int32."""
    g = grey8(color)
    s = eligible_score(g, depth, threshold)
    return g, box5(g), cell_slots(s, nms(s), cell)


def direction_table():
    a = 2.0 * np.pi * np.arange(BINS) / BINS
    return np.rint(16384.0 * np.stack([np.cos(a), np.sin(a)], axis=1)).astype(np.int32)


def rotated_patterns(pattern=PATTERN):
    p = np.asarray(pattern, dtype=np.float64).reshape(256, 2, 2)
    out = np.empty((BINS, 256, 4), dtype=np.int8)
    for k in range(BINS):
        c, s = np.cos(2.0 * np.pi * k / BINS), np.sin(2.0 * np.pi * k / BINS)
        out[k, :, 0::2] = np.rint(c * p[..., 0] - s * p[..., 1])
        out[k, :, 1::2] = np.rint(s * p[..., 0] + c * p[..., 1])
    return out


_DISC = [(dx, dy) for dy in range(-RADIUS, RADIUS + 1) for dx in range(-RADIUS, RADIUS + 1) if dx * dx + dy * dy <= RADIUS * RADIUS]


def moments(g8, x, y):
    m10 = sum(dx * int(g8[y + dy, x + dx]) for dx, dy in _DISC)
    m01 = sum(dy * int(g8[y + dy, x + dx]) for dx, dy in _DISC)
    return m10, m01


def orientation_bin(m10, m01, dirs=None):
    dirs = direction_table() if dirs is None else dirs
    v = dirs[:, 0].astype(np.int64) * np.int64(m10) + dirs[:, 1].astype(np.int64) * np.int64(m01)
    return int(np.argmax(v))


def describe(g8, box, slots, oriented=True, tables=None, dirs=None):
    """-> slots with the bins filled in, desc [cells, 8] uint32 (zeros for an empty slot)."""
    tables = rotated_patterns() if tables is None else tables
    dirs = direction_table() if dirs is None else dirs
    out = slots.copy()
    desc = np.zeros((slots.shape[0], 8), dtype=np.uint32)
    for n, (x, y, sc, _) in enumerate(slots):
        if sc <= 0:
            continue
        k = orientation_bin(*moments(g8, int(x), int(y)), dirs) if oriented else 0
        out[n, 3] = k
        t = tables[k].astype(np.int64)
        bits = box[y + t[:, 1], x + t[:, 0]] < box[y + t[:, 3], x + t[:, 2]]
        for i in np.nonzero(bits)[0]:
            desc[n, i // 32] |= np.uint32(1) << np.uint32(i % 32)
    return out, desc


def detect_and_describe(color, depth, threshold=20, cell=16, oriented=True):
    """-> {"g8", "box5", "slots", "slot_desc", and the keypoints "x", "y", "score", "bin", "desc"}."""
    g, b, slots = detect(color, depth, threshold, cell)
    slots, desc = describe(g, b, slots, oriented)
    live = slots[:, 2] > 0
    return {"g8": g, "box5": b, "slots": slots, "slot_desc": desc, "x": slots[live, 0], "y": slots[live, 1], "score": slots[live, 2],
            "bin": slots[live, 3], "desc": desc[live]}


def hamming(q, r):
    """[Q, 8] x [R, 8] uint32 -> [Q, R] int64."""
    x = (np.asarray(q, dtype=np.uint32)[:, None, :] ^ np.asarray(r, dtype=np.uint32)[None, :, :])
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=-1).sum(axis=-1).astype(np.int64).reshape(len(q), len(r))


def match(q, r):
    """-> [Q, 3] int32: index, distance, second."""
    Q, R = len(q), len(r)
    out = np.empty((Q, 3), dtype=np.int32)
    out[:] = (-1, NO_MATCH, NO_MATCH)
    if Q == 0 or R == 0:
        return out
    d = hamming(q, r)
    best = np.argmin(d, axis=1)                                       # the first of equal minima
    out[:, 0], out[:, 1] = best, d[np.arange(Q), best]
    if R > 1:
        d[np.arange(Q), best] = NO_MATCH
        out[:, 2] = d.min(axis=1)
    return out


def filter_matches(m_ba, m_ab, max_hamming=64, ratio=0.8):
    """m_ba: b's keypoints against a's, m_ab the other way -> [(i in b, j in a, d)]."""
    out = []
    for i, (j, d, second) in enumerate(np.asarray(m_ba).tolist()):
        if j >= 0 and m_ab[j][0] == i and d <= max_hamming and d <= float(ratio) * second:
            out.append((i, int(j), int(d)))
    return out


def mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def kabsch(pb, pa):
    """R, t with pa ~ R pb + t (float64)."""
    cb, ca = pb.mean(axis=0), pa.mean(axis=0)
    U, _, Vt = np.linalg.svd((pa - ca).T @ (pb - cb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ D @ Vt
    return R, ca - R @ cb


def _spread(p):
    e1, e2 = p[1] - p[0], p[2] - p[0]
    n1, n2 = np.linalg.norm(e1), np.linalg.norm(e2)
    return n1 > 1e-9 and n2 > 1e-9 and np.linalg.norm(np.cross(e1, e2)) >= 0.1 * n1 * n2


def ransac_rigid(pa, pb, iters=512, inlier_dist=0.05, seed=0):
    pa, pb = np.asarray(pa, dtype=np.float64).reshape(-1, 3), np.asarray(pb, dtype=np.float64).reshape(-1, 3)
    n = pa.shape[0]
    if n < 3 or pb.shape[0] != n:
        return None
    count = lambda R, t: np.linalg.norm(pb @ R.T + t - pa, axis=1) <= inlier_dist
    best = None
    for h in range(int(iters)):
        idx = [mix32(int(seed) + 3 * h + j) % n for j in range(3)]
        if len(set(idx)) < 3 or not _spread(pa[idx]) or not _spread(pb[idx]):
            continue
        R, t = kabsch(pb[idx], pa[idx])
        mask = count(R, t)
        if best is None or mask.sum() > best[2].sum():
            best = (R, t, mask)
    if best is None:
        return None
    R, t, mask = best
    for _ in range(3):
        if mask.sum() < 3:
            break
        R2, t2 = kabsch(pb[mask], pa[mask])
        m2 = count(R2, t2)
        if m2.sum() < mask.sum():
            break
        same = np.array_equal(m2, mask)
        R, t, mask = R2, t2, m2
        if same:
            break
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    res = np.linalg.norm(pb[mask] @ R.T + t - pa[mask], axis=1)
    return T, mask, float(np.sqrt(np.mean(res ** 2))) if mask.any() else 0.0


def backproject(x, y, depth_hw, K):
    """The keypoints' pixels with the keyframe's depth [H, W] and K -> [N, 3] float64 in the camera's frame."""
    x, y, K = np.asarray(x), np.asarray(y), np.asarray(K, dtype=np.float64)
    z = np.asarray(depth_hw, dtype=np.float64)[y, x]
    return np.stack([(x - K[0, 2]) / K[0, 0] * z, (y - K[1, 2]) / K[1, 1] * z, z], axis=1)
