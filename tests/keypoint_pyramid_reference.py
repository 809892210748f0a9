"""The definition of the keypoints over an image pyramid and of the keypoint votes (csrc/keypoint_pyramid.hip,
rtg_slam_amd/keypoints.py) in numpy, on top of tests/keypoint_reference.py, which it uses and does not change.  Everything after
level 0's grey value is integer arithmetic: the kernels match this file bit for bit.

THE LADDER.  SCALES lists num / den of level l: 1, 3/2, 2, 3, 4.  Level 1 is level 0 reduced 3:2 (reduce32), level 2 is level 0
reduced 2:1 (reduce2), level 3 is level 1 reduced 2:1, level 4 is level 2 reduced 2:1.
    2:1  size floor(W / 2) x floor(H / 2), value (a + b + c + d + 2) >> 2 of the 2 x 2 block; a trailing odd row or column is dropped.
    3:2  size 2 floor(W / 3) x 2 floor(H / 3).  Along each axis output 2k takes the inputs 3k, 3k + 1 with the weights 2, 1 and
         output 2k + 1 the inputs 3k + 1, 3k + 2 with 1, 2; value (sum of the 2-D weight products times g8 + 4) // 9.
Level 0's g8 is keypoint_reference.grey8.

LEVEL DEPTH.  A level's depth at (x, y) is level 0's at (floor((2x + 1) num / (2 den)), floor((2y + 1) num / (2 den))), the pixel
under the level pixel's centre.  Nothing is averaged, so nothing invalid is mixed in.

WHICH LEVELS.  Level 0 is always used.  A later level is dropped, with every level after it, when its image cannot hold one cell
inside the 16-pixel margin: W_l < 32 + cell or H_l < 32 + cell (level_table).  "levels_used" says how many are left.

PER LEVEL the rule is keypoint_reference's, unchanged, in the level's own pixels: FAST-9 score, threshold, margin, 3 x 3 suppression,
one slot per cell, orientation, pattern tables, descriptor.  The slots of the levels follow each other, level 0 first; the
keypoints are the non-empty slots in that order, "level" says where each came from.

LEVEL-0 POSITION.  x0 = (x + 0.5) s - 0.5, y0 likewise, s = num / den, in float64.  A keypoint is back-projected at (x0, y0) with
the level depth of its own pixel (backproject).

VOTES of a pair (a, b) from the two match tables: len(keypoint_reference.filter_matches(m_ba, m_ab, max_hamming, ratio)).

SHORTLIST (top_k).  Of the counts of one keyframe's older partners the k highest that reach `floor`, a tie going to the lower
index; in order of descending count."""
import numpy as np

from tests import keypoint_reference as ref

F32 = np.float32
MAX_LEVELS = 5
SCALES = ((1, 1), (3, 2), (2, 1), (3, 1), (4, 1))
PARENT = (None, 0, 0, 1, 2)


def reduce2(g):
    H, W = g.shape
    h, w = H // 2, W // 2
    v = g[:2 * h, :2 * w].astype(np.int32)
    return ((v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def _reduce32_rows(v):
    """[3k, n] int32 -> [2k, n]: rows 2k = 2 v[3k] + v[3k + 1], rows 2k + 1 = v[3k + 1] + 2 v[3k + 2] (weights not yet divided)."""
    out = np.empty((2 * (v.shape[0] // 3), v.shape[1]), dtype=np.int32)
    out[0::2] = 2 * v[0::3] + v[1::3]
    out[1::2] = v[1::3] + 2 * v[2::3]
    return out


def reduce32(g):
    H, W = g.shape
    h, w = H // 3, W // 3
    v = g[:3 * h, :3 * w].astype(np.int32)
    s = _reduce32_rows(_reduce32_rows(v).T).T
    return ((s + 4) // 9).astype(np.uint8)


def level_sizes(H, W, levels):
    """[(H_l, W_l)] of the first `levels` levels of the ladder, whatever their size."""
    out = [(int(H), int(W))]
    for l in range(1, int(levels)):
        ph, pw = out[PARENT[l]]
        out.append((2 * (ph // 3), 2 * (pw // 3)) if l == 1 else (ph // 2, pw // 2))
    return out


def level_table(H, W, levels, cell=None):
    """-> int32 [levels_used, 5]: first pixel of the level in the buffers (the levels packed one after the other), H, W, num, den.
    With a cell the levels that cannot hold one cell inside the margin are dropped, and all after them; without one only empty
    levels are."""
    if not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError("levels must lie in 1 .. 5")
    rows, off = [], 0
    for l, (h, w) in enumerate(level_sizes(H, W, levels)):
        need = 1 if cell is None else 2 * ref.MARGIN + int(cell)
        if l > 0 and (h < need or w < need):
            break
        rows.append((off, h, w) + SCALES[l])
        off += h * w
    return np.asarray(rows, dtype=np.int32).reshape(-1, 5)


def level_depth(depth, h, w, num, den):
    z = np.asarray(depth, dtype=F32)
    H, W = z.shape[-2], z.shape[-1]
    z = z.reshape(H, W)
    ys = ((2 * np.arange(h) + 1) * num) // (2 * den)
    xs = ((2 * np.arange(w) + 1) * num) // (2 * den)
    return z[np.ix_(ys, xs)]


def pyramid(color, depth, table):
    """-> [(g8 [H_l, W_l] uint8, depth [H_l, W_l] float32)] for the rows of `table`."""
    g = [ref.grey8(color)]
    for l in range(1, len(table)):
        g.append(reduce32(g[0]) if l == 1 else reduce2(g[PARENT[l]]))
    out = []
    for l, (_, h, w, num, den) in enumerate(np.asarray(table).tolist()):
        assert g[l].shape == (h, w), (l, g[l].shape, h, w)
        out.append((g[l], level_depth(depth, h, w, num, den)))
    return out


def packed(planes, table, dtype):
    """The per-level planes in one buffer, as the kernels hold them."""
    t = np.asarray(table)
    buf = np.zeros(int(t[-1, 0] + t[-1, 1] * t[-1, 2]), dtype=dtype)
    for p, (off, h, w, _, _) in zip(planes, t.tolist()):
        buf[off:off + h * w] = np.asarray(p).reshape(-1)
    return buf


def detect_and_describe(color, depth, threshold=20, cell=16, oriented=True, levels=1, table=None):
    """-> {"table", "levels_used", per level "g8", "depth", "box5" (lists); "slots" [cells, 4], "slot_desc" [cells, 8], "slot_level"
    [cells]; and the keypoints "x", "y", "score", "bin", "desc", "level", "x0", "y0" (float64)}.  `table`: the levels to use instead
    of level_table(H, W, levels, cell)."""
    H, W = np.asarray(color).shape[-2:]
    table = level_table(H, W, levels, cell) if table is None else np.asarray(table, dtype=np.int32)
    pyr = pyramid(color, depth, table)
    slots, descs, boxes, lev = [], [], [], []
    for l, (g, z) in enumerate(pyr):
        s = ref.eligible_score(g, z, threshold)
        b = ref.box5(g)
        sl, d = ref.describe(g, b, ref.cell_slots(s, ref.nms(s), cell), oriented)
        slots.append(sl)
        descs.append(d)
        boxes.append(b)
        lev.append(np.full(len(sl), l, dtype=np.int32))
    slots, descs, lev = np.concatenate(slots), np.concatenate(descs), np.concatenate(lev)
    live = slots[:, 2] > 0
    scale = np.array([num / den for _, _, _, num, den in table.tolist()], dtype=np.float64)[lev[live]]
    x, y = slots[live, 0], slots[live, 1]
    return {"table": table, "levels_used": len(table), "g8": [p[0] for p in pyr], "depth": [p[1] for p in pyr], "box5": boxes,
            "slots": slots, "slot_desc": descs, "slot_level": lev, "x": x, "y": y, "score": slots[live, 2], "bin": slots[live, 3],
            "desc": descs[live], "level": lev[live], "x0": (x + 0.5) * scale - 0.5, "y0": (y + 0.5) * scale - 0.5}


def backproject(f, K):
    """The keypoints of detect_and_describe at (x0, y0) with the level depth of their own pixel -> [N, 3] float64."""
    K = np.asarray(K, dtype=np.float64)
    z = np.array([f["depth"][l][y, x] for l, x, y in zip(f["level"].tolist(), f["x"].tolist(), f["y"].tolist())], dtype=np.float64).reshape(-1)
    return np.stack([(f["x0"] - K[0, 2]) / K[0, 0] * z, (f["y0"] - K[1, 2]) / K[1, 1] * z, z], axis=1)


def votes(m_ba, m_ab, max_hamming=64, ratio=0.8):
    return len(ref.filter_matches(m_ba, m_ab, max_hamming, ratio))


def top_k(counts, k, floor):
    """counts[a] of the older keyframes a = 0 .. -> the indices of the k highest counts >= floor, ties to the lower index, in
    order of descending count."""
    order = sorted((a for a, c in enumerate(counts) if c >= floor), key=lambda a: (-int(counts[a]), a))
    return order[:int(k)]
