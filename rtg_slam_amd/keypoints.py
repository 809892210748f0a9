"""A relative pose for a candidate pair of keyframes from the two frames alone (csrc/keypoints.hip; the definition is
tests/keypoint_reference.py): what the reference gets from its ORB back end, in its smallest sound form.

    detect_and_describe   a keyframe's colour and depth -> its keypoints (rtgs_keypoint_detect, rtgs_keypoint_describe)
    match_pairs           a batch of (query keyframe, reference keyframe) pairs in ONE launch (rtgs_keypoint_match)
    filter_matches        mutual best, Hamming bound, ratio test (host)
    ransac_rigid          3-D - 3-D RANSAC over the matches' back-projected points (host, numpy float64, deterministic)
    relative_pose         the four together for one pair -> T = T_a^-1 T_b with its count of geometric witnesses, or a refusal
    rigid_ransac_pairs    the filter and the RANSAC of a batch of pairs on the device, ONE launch behind the match launch, the match
                          tables never leaving the device (rtgs_rigid_ransac; the definition is tests/rigid_ransac_reference.py)
    vote_pairs            the number of filtered matches of a batch of pairs: ONE launch behind the match launch, only the counts
                          leave the device (rtgs_keypoint_votes)

FAST-9 corners on the 8-bit grey image, one per cell of the image, oriented by the intensity centroid in 32 bins, described by
256 comparisons of 5 x 5 box sums.  Pixel-centre localisation, no vocabulary.  Single scale by default; with the option `levels`
(2 .. 5) the same rule runs on every level of an image pyramid of the scales 1, 3/2, 2, 3, 4 (csrc/keypoint_pyramid.hip; the
definition is tests/keypoint_pyramid_reference.py), three launches a frame whatever the number of levels, and a keypoint of a
coarser level is back-projected at the level-0 position of its pixel's centre with that pixel's own depth.  After the grey
value everything on the device is integer arithmetic, so the kernels match the definition bit for bit.  There is no fallback: a
CPU tensor or a missing kernel is an error."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .keypoint_pattern import PATTERN

MARGIN = _lib.CONSTANTS["RTGS_KEYPOINT_MARGIN"]
MIN_CELL, MAX_CELL = _lib.CONSTANTS["RTGS_KEYPOINT_MIN_CELL"], _lib.CONSTANTS["RTGS_KEYPOINT_MAX_CELL"]
BINS = 32
MAX_LEVELS = _lib.CONSTANTS["RTGS_KEYPOINT_MAX_LEVELS"]
SCALES = ((1, 1), (3, 2), (2, 1), (3, 1), (4, 1))                  # num / den of level l; level 3 is level 1 halved, level 4 level 2
# the loop closure's loop_closure_keypoint_* keys (loop_closure.DEFAULTS takes them from here); chosen on the synthetic textured
# box room, none measured on real data
DEFAULTS = {
    "threshold": 20,            # FAST-9 score a corner must exceed: an absolute contrast of the 8-bit grey image
    "cell": 16,                 # pixels: one keypoint per cell x cell pixels
    "oriented": True,           # False: bin 0 for every keypoint (no in-plane rotation between the views)
    "max_hamming": 64,          # of 256 bits
    "ratio": 0.8,               # best distance <= ratio x second best
    "ransac_iters": 512,
    "inlier_dist": 0.05,        # metres: half of icp_distance_threshold - the dense registration only needs to start inside its gates
    "min_inliers": 8,           # three define the hypothesis; wrong pairs of the textured room end with at most 2, right ones with 18+
}


def config(**over) -> SimpleNamespace:
    """The keypoint options as a namespace, validated.  Raises ValueError."""
    unknown = set(over) - set(DEFAULTS) - {"levels"}
    if unknown:
        raise ValueError(f"keypoints: unknown option {sorted(unknown)[0]}")
    v = dict(DEFAULTS, **over)
    cfg = SimpleNamespace(threshold=int(v["threshold"]), cell=int(v["cell"]), oriented=bool(v["oriented"]), max_hamming=int(v["max_hamming"]),
                          ratio=float(v["ratio"]), ransac_iters=int(v["ransac_iters"]), inlier_dist=float(v["inlier_dist"]),
                          min_inliers=int(v["min_inliers"]))
    if not 0 <= cfg.threshold <= 255:
        raise ValueError("loop_closure_keypoint_threshold must lie in 0 .. 255")
    if not MIN_CELL <= cfg.cell <= MAX_CELL:
        raise ValueError(f"loop_closure_keypoint_cell must lie in {MIN_CELL} .. {MAX_CELL}")
    if not 0 <= cfg.max_hamming <= 256:
        raise ValueError("loop_closure_keypoint_max_hamming must lie in 0 .. 256")
    if not 0 < cfg.ratio <= 1:
        raise ValueError("loop_closure_keypoint_ratio must lie in (0, 1]")
    if cfg.ransac_iters < 1:
        raise ValueError("loop_closure_keypoint_ransac_iters must be >= 1")
    if not cfg.inlier_dist > 0:
        raise ValueError("loop_closure_keypoint_inlier_dist must be positive")
    if cfg.min_inliers < 3:
        raise ValueError("loop_closure_keypoint_min_inliers must be >= 3: three pairs define the pose")
    if "levels" in over:                                            # kept out of DEFAULTS: absent, no namespace and no report knows of it
        if isinstance(over["levels"], bool) or int(over["levels"]) != over["levels"] or not 1 <= int(over["levels"]) <= MAX_LEVELS:
            raise ValueError(f"loop_closure_keypoint_levels must be an integer in 1 .. {MAX_LEVELS}")
        cfg.levels = int(over["levels"])
    return cfg


def level_table(H: int, W: int, levels: int, cell: int) -> np.ndarray:
    """The levels of an H x W frame's pyramid -> int32 [levels used, 5]: first pixel in the packed buffers, H_l, W_l, num, den.
    Level 1 is level 0 reduced 3:2 (2 floor(n / 3)), levels 2, 3, 4 are levels 0, 1, 2 halved (floor(n / 2)).  Level 0 is always
    there; a later level whose image cannot hold one cell inside the margin (a side below 2 MARGIN + cell) is dropped, and all
    after it."""
    sizes, rows, off = [(int(H), int(W))], [], 0
    for l in range(1, int(levels)):
        ph, pw = sizes[0 if l < 3 else l - 2]
        sizes.append((2 * (ph // 3), 2 * (pw // 3)) if l == 1 else (ph // 2, pw // 2))
    for l, (h, w) in enumerate(sizes):
        if l > 0 and min(h, w) < 2 * MARGIN + int(cell):
            break
        rows.append((off, h, w) + SCALES[l])
        off += h * w
    return np.asarray(rows, dtype=np.int32).reshape(-1, 5)


def direction_table() -> np.ndarray:
    """[32, 2] int32: rint(16384 (cos, sin)(2 pi k / 32))."""
    a = 2.0 * np.pi * np.arange(BINS) / BINS
    return np.rint(16384.0 * np.stack([np.cos(a), np.sin(a)], axis=1)).astype(np.int32)


def rotated_patterns() -> np.ndarray:
    """[32, 256, 4] int8: PATTERN turned into every bin, rint(R_k p) in float64."""
    p = np.asarray(PATTERN, dtype=np.float64).reshape(256, 2, 2)
    out = np.empty((BINS, 256, 4), dtype=np.int8)
    for k in range(BINS):
        c, s = np.cos(2.0 * np.pi * k / BINS), np.sin(2.0 * np.pi * k / BINS)
        out[k, :, 0::2] = np.rint(c * p[..., 0] - s * p[..., 1])
        out[k, :, 1::2] = np.rint(s * p[..., 0] + c * p[..., 1])
    return out


_tables: Dict = {}


def _device_tables(dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dirs [32, 2] int32, tables [32, 256] int32 - the four int8 of a pair packed, lowest byte first) on `dev`, built once."""
    key = (dev.type, dev.index)
    if key not in _tables:
        packed = np.ascontiguousarray(rotated_patterns()).view("<i4").reshape(BINS, 256)
        _tables[key] = (torch.from_numpy(direction_table()).to(dev), torch.from_numpy(packed.astype(np.int32)).to(dev))
    return _tables[key]


def _check_image(color_chw, depth_chw):
    if not (torch.is_tensor(color_chw) and color_chw.is_cuda and color_chw.dtype == torch.float32 and color_chw.dim() == 3
            and color_chw.shape[0] == 3):
        raise ValueError("keypoints: colour must be a float32 [3, H, W] tensor on the device")
    H, W = int(color_chw.shape[1]), int(color_chw.shape[2])
    if not (torch.is_tensor(depth_chw) and depth_chw.device == color_chw.device and depth_chw.dtype == torch.float32
            and depth_chw.numel() == H * W):
        raise ValueError("keypoints: depth must be a float32 [1, H, W] tensor on the colour's device")
    return H, W


def detect_and_describe(color_chw: torch.Tensor, depth_chw: torch.Tensor, K, cfg=None, keep_planes: bool = False) -> Dict:
    """-> {"x", "y", "score", "bin": int32 numpy [N]; "desc": int32 [N, 8] on the device (the uint32 words' bits); "xyz": float64
    numpy [N, 3], the pixels back-projected with the depth and K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]}, the keypoints in slot
    order.  With keep_planes also "g8" (uint8 [H, W]), "box5" (int32 [H, W]), "slots" (int32 [cells, 4]) and "slot_desc" (int32
    [cells, 8]) on the device, as the kernels left them.  Two launches and one small copy to the host (the slots).
    With cfg.levels above 1 see _detect_and_describe_levels: three launches, and the dict gains "level", "x0", "y0", "levels_used"."""
    cfg = config() if cfg is None else cfg
    H, W = _check_image(color_chw, depth_chw)
    if getattr(cfg, "levels", 1) > 1:
        return _detect_and_describe_levels(color_chw, depth_chw, H, W, K, cfg, keep_planes)
    dev = color_chw.device
    c = int(cfg.cell)
    n_slots = (-(-W // c)) * (-(-H // c))
    color_chw, depth_chw = color_chw.contiguous(), depth_chw.contiguous()
    g8 = torch.empty((H, W), dtype=torch.uint8, device=dev)
    box = torch.empty((H, W), dtype=torch.int32, device=dev)
    slots = torch.empty((n_slots, 4), dtype=torch.int32, device=dev)
    slot_desc = torch.empty((n_slots, 8), dtype=torch.int32, device=dev)
    dirs, tables = _device_tables(dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.rtgs_keypoint_detect(_lib.ptr(color_chw), _lib.ptr(depth_chw), H, W, c, int(cfg.threshold), _lib.ptr(g8), _lib.ptr(box),
                                      _lib.ptr(slots), _lib.stream(dev))
        _lib.check(rc, "rtgs_keypoint_detect")
        rc = lib.rtgs_keypoint_describe(_lib.ptr(g8), _lib.ptr(box), H, W, n_slots, int(bool(cfg.oriented)), _lib.ptr(dirs),
                                        _lib.ptr(tables), _lib.ptr(slots), _lib.ptr(slot_desc), _lib.stream(dev))
        _lib.check(rc, "rtgs_keypoint_describe")
    live = torch.nonzero(slots[:, 2] > 0).reshape(-1)
    kp = slots[live]
    z = depth_chw.reshape(H, W)[kp[:, 1].long(), kp[:, 0].long()]
    host = torch.cat([kp.to(torch.float64), z.to(torch.float64)[:, None]], dim=1).cpu().numpy()      # the one copy
    Kn = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64)
    x, y, zz = host[:, 0], host[:, 1], host[:, 4]
    out = {"x": host[:, 0].astype(np.int32), "y": host[:, 1].astype(np.int32), "score": host[:, 2].astype(np.int32),
           "bin": host[:, 3].astype(np.int32), "desc": slot_desc[live].contiguous(),
           "xyz": np.stack([(x - Kn[0, 2]) / Kn[0, 0] * zz, (y - Kn[1, 2]) / Kn[1, 1] * zz, zz], axis=1)}
    if keep_planes:
        out.update(g8=g8, box5=box, slots=slots, slot_desc=slot_desc)
    return out


_geometry: Dict = {}


def _level_geometry(H, W, levels, cell, dev):
    """What depends on the frame's size alone, built once per device: the level table (host), the pixel and slot totals and, on
    the device, each slot's level, first pixel and row length."""
    key = (H, W, levels, cell, dev.type, dev.index)
    if key not in _geometry:
        table = level_table(H, W, levels, cell)
        cells = [(-(-int(h) // cell)) * (-(-int(w) // cell)) for _, h, w, _, _ in table]
        lev = np.repeat(np.arange(len(table)), cells)
        _geometry[key] = SimpleNamespace(table=np.ascontiguousarray(table), n_pixels=int(table[-1, 0] + table[-1, 1] * table[-1, 2]),
                                         n_slots=int(sum(cells)), slot_level=torch.from_numpy(lev.astype(np.int64)).to(dev),
                                         slot_off=torch.from_numpy(table[lev, 0].astype(np.int64)).to(dev),
                                         slot_w=torch.from_numpy(table[lev, 2].astype(np.int64)).to(dev))
    return _geometry[key]


def _detect_and_describe_levels(color_chw, depth_chw, H, W, K, cfg, keep_planes) -> Dict:
    """detect_and_describe over cfg.levels levels of the pyramid (level_table): rtgs_keypoint_pyramid, rtgs_keypoint_detect_levels
    and rtgs_keypoint_describe_levels, three launches whatever the number of levels, and one small copy to the host.  The
    keypoints are the non-empty slots of level 0 in slot order, then level 1's, and so on; "x", "y" are in the pixels of the
    keypoint's "level", "x0" = (x + 0.5) s - 0.5 and "y0" (float64, s the level's scale) the position in level 0, at which "xyz" is
    back-projected with the level depth of the keypoint's own pixel.  "levels_used" counts the levels that were not dropped.
    With keep_planes the planes are the packed buffers of all levels and "table" the level table."""
    dev = color_chw.device
    c = int(cfg.cell)
    geo = _level_geometry(H, W, int(cfg.levels), c, dev)
    n, total = len(geo.table), geo.n_pixels
    color_chw, depth_chw = color_chw.contiguous(), depth_chw.contiguous()
    g8 = torch.empty((total,), dtype=torch.uint8, device=dev)
    dl = torch.empty((total,), dtype=torch.float32, device=dev)
    box = torch.empty((total,), dtype=torch.int32, device=dev)
    slots = torch.empty((geo.n_slots, 4), dtype=torch.int32, device=dev)
    slot_desc = torch.empty((geo.n_slots, 8), dtype=torch.int32, device=dev)
    dirs, tables = _device_tables(dev)
    lib = _lib.load()
    levels = geo.table.ctypes.data                                   # a host array: the entry points read it before they launch
    with torch.cuda.device(dev):
        rc = lib.rtgs_keypoint_pyramid(_lib.ptr(color_chw), _lib.ptr(depth_chw), levels, n, total, _lib.ptr(g8), _lib.ptr(dl), _lib.stream(dev))
        _lib.check(rc, "rtgs_keypoint_pyramid")
        rc = lib.rtgs_keypoint_detect_levels(_lib.ptr(g8), _lib.ptr(dl), levels, n, total, c, int(cfg.threshold), _lib.ptr(box), _lib.ptr(slots),
                                             _lib.stream(dev))
        _lib.check(rc, "rtgs_keypoint_detect_levels")
        rc = lib.rtgs_keypoint_describe_levels(_lib.ptr(g8), _lib.ptr(box), levels, n, total, c, int(bool(cfg.oriented)), _lib.ptr(dirs),
                                               _lib.ptr(tables), _lib.ptr(slots), _lib.ptr(slot_desc), _lib.stream(dev))
        _lib.check(rc, "rtgs_keypoint_describe_levels")
    live = torch.nonzero(slots[:, 2] > 0).reshape(-1)
    kp = slots[live]
    z = dl[geo.slot_off[live] + kp[:, 1].long() * geo.slot_w[live] + kp[:, 0].long()]
    host = torch.cat([kp.to(torch.float64), z.to(torch.float64)[:, None], geo.slot_level[live].to(torch.float64)[:, None]], dim=1).cpu().numpy()
    Kn = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64)
    level = host[:, 5].astype(np.int32)
    scale = np.array([num / den for num, den in SCALES], dtype=np.float64)[level]
    x0, y0, zz = (host[:, 0] + 0.5) * scale - 0.5, (host[:, 1] + 0.5) * scale - 0.5, host[:, 4]
    out = {"x": host[:, 0].astype(np.int32), "y": host[:, 1].astype(np.int32), "score": host[:, 2].astype(np.int32),
           "bin": host[:, 3].astype(np.int32), "desc": slot_desc[live].contiguous(), "level": level, "x0": x0, "y0": y0,
           "levels_used": n, "xyz": np.stack([(x0 - Kn[0, 2]) / Kn[0, 0] * zz, (y0 - Kn[1, 2]) / Kn[1, 1] * zz, zz], axis=1)}
    if keep_planes:
        out.update(g8=g8, depth_levels=dl, box5=box, slots=slots, slot_desc=slot_desc, table=geo.table.copy())
    return out


def _match_launch(features, pairs):
    """The launch of match_pairs -> (out int32 [n_out, 3] on the device, or None when there is no query at all; table: per pair
    (first query row, query count, first reference row, reference count, first row of out))."""
    keys = list(dict.fromkeys(k for pair in pairs for k in pair))   # in order of first appearance
    descs = [features[k]["desc"] for k in keys]
    for d in descs:
        if not (torch.is_tensor(d) and d.is_cuda and d.dtype == torch.int32 and d.dim() == 2 and d.shape[1] == 8
                and d.device == descs[0].device):
            raise ValueError("match_pairs: every descriptor set must be an int32 [N, 8] tensor on one device")
    dev = descs[0].device
    begin, total = {}, 0
    for k, d in zip(keys, descs):
        begin[k] = total
        total += int(d.shape[0])
    table, n_out = [], 0
    for q, r in pairs:
        nq = int(features[q]["desc"].shape[0])
        table.append((begin[q], nq, begin[r], int(features[r]["desc"].shape[0]), n_out))
        n_out += nq
    if n_out == 0:
        return None, table
    if len(pairs) > 65535:
        raise ValueError("match_pairs: at most 65535 pairs a launch")
    all_desc = torch.cat(descs, dim=0).contiguous()
    out = torch.empty((n_out, 3), dtype=torch.int32, device=dev)
    tab = torch.tensor(table, dtype=torch.int32).to(dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.rtgs_keypoint_match(_lib.ptr(all_desc), total, _lib.ptr(tab), len(pairs), max(t[1] for t in table), _lib.ptr(out), n_out,
                                     _lib.stream(dev))
    _lib.check(rc, "rtgs_keypoint_match")
    return out, table


def match_pairs(features, pairs: Sequence[Tuple]) -> List[np.ndarray]:
    """features: keyframe key -> {"desc": int32 [N, 8] on the device} (a dict, or a list indexed by key); pairs: [(query key,
    reference key)] -> per pair an int32 numpy [N_query, 3]: the reference's index, the distance, the second distance (-1, 257,
    257 against an empty set).  One launch and one copy to the host for the whole batch."""
    pairs = list(pairs)
    if not pairs:
        return []
    out, table = _match_launch(features, pairs)
    if out is None:
        return [np.empty((0, 3), dtype=np.int32) for _ in pairs]
    host = out.cpu().numpy()
    return [host[t[4]:t[4] + t[1]] for t in table]


def match_pairs_device(features, pairs: Sequence[Tuple]) -> Tuple:
    """match_pairs with its table left on the device, for rigid_ransac_tables: -> (int32 [n_out, 3] device tensor, or None
    when no pair has a query; [(first row, rows)] per pair).  One launch, no copy to the host."""
    pairs = list(pairs)
    if not pairs:
        return None, []
    out, table = _match_launch(features, pairs)
    return out, [(t[4], t[1]) for t in table]


def filter_matches(m_ba, m_ab, max_hamming: int = 64, ratio: float = 0.8) -> List[Tuple[int, int, int]]:
    """m_ba: b's keypoints matched against a's, m_ab the other way (rows of match_pairs) -> [(i in b, j in a, distance)] in
    order of i: each the other's best, distance <= max_hamming and <= ratio x the second best on b's side."""
    out = []
    m_ab = np.asarray(m_ab)
    for i, (j, d, second) in enumerate(np.asarray(m_ba).tolist()):
        if j >= 0 and int(m_ab[j][0]) == i and d <= max_hamming and d <= float(ratio) * second:
            out.append((i, int(j), int(d)))
    return out


def mix32(x: int) -> int:
    """The counter-based generator of ransac_rigid: a 32-bit integer hash, no state."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def kabsch(pb, pa):
    """R, t (float64) with pa ~ R pb + t in the least-squares sense."""
    cb, ca = pb.mean(axis=0), pa.mean(axis=0)
    U, _, Vt = np.linalg.svd((pa - ca).T @ (pb - cb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ D @ Vt
    return R, ca - R @ cb


def _spread(p) -> bool:
    e1, e2 = p[1] - p[0], p[2] - p[0]
    n1, n2 = np.linalg.norm(e1), np.linalg.norm(e2)
    return bool(n1 > 1e-9 and n2 > 1e-9 and np.linalg.norm(np.cross(e1, e2)) >= 0.1 * n1 * n2)


def ransac_rigid(pa, pb, iters: int = 512, inlier_dist: float = 0.05, seed: int = 0):
    """Matched 3-D points pa [n, 3] (in a's camera) and pb [n, 3] (in b's) -> (T 4 x 4 float64 with p_a = T p_b, that is
    T_a^-1 T_b; the inliers' mask; the rms of their residuals) or None (fewer than 3 matches, no valid triplet).  Hypothesis h
    draws the indices mix32(seed + 3 h + j) mod n, j = 0, 1, 2; a triplet with a repeated index, or whose angle at its first
    point lies below 5.74 or above 174.26 degrees in either frame (|e1 x e2| < 0.1 |e1| |e2|), is skipped; the highest inlier
    count wins, the earliest on a tie; then up to three rounds of refitting on the inliers, a round that loses inliers dropped."""
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


def pose_from_matches(features_a: Dict, features_b: Dict, m_ba, m_ab, cfg) -> Dict:
    """The host half of relative_pose, from the two match tables of match_pairs."""
    out = {"T": None, "inliers": 0, "matches": 0, "rms": None, "keypoints_a": int(len(features_a["x"])),
           "keypoints_b": int(len(features_b["x"])), "reason": None}
    m = filter_matches(m_ba, m_ab, cfg.max_hamming, cfg.ratio)
    out["matches"] = len(m)
    fit = None
    if len(m) >= 3:
        fit = ransac_rigid(features_a["xyz"][[j for _, j, _ in m]], features_b["xyz"][[i for i, _, _ in m]], cfg.ransac_iters,
                           cfg.inlier_dist)
    if fit is not None:
        out["inliers"], out["rms"] = int(fit[1].sum()), fit[2]
    if out["inliers"] < cfg.min_inliers:                          # also: fewer than 3 matches, no valid triplet (0 inliers)
        out["reason"] = f"{out['inliers']} inliers of {len(m)} matches, below {cfg.min_inliers}"
        return out
    out["T"] = fit[0]
    return out


def relative_pose(features_a: Dict, features_b: Dict, cfg=None) -> Dict:
    """The two keyframes' features (detect_and_describe) -> {"T": T_a^-1 T_b in loop_closure.register_pair's convention (4 x 4
    float64), "inliers", "matches", "rms" (metres), "keypoints_a", "keypoints_b", "reason": None} - or a refusal: "T" None and
    "reason" "k inliers of n matches, below m" (k = 0 with fewer than 3 matches or without a valid triplet).  One match launch, both directions."""
    cfg = config() if cfg is None else cfg
    m_ba, m_ab = match_pairs({"a": features_a, "b": features_b}, [("b", "a"), ("a", "b")])
    return pose_from_matches(features_a, features_b, m_ba, m_ab, cfg)


RANSAC_CAP, RANSAC_HEAD = _lib.CONSTANTS["RTGS_RANSAC_MAX_MATCHES"], _lib.CONSTANTS["RTGS_RANSAC_HEAD"]
RANSAC_MAX_ITERS = _lib.CONSTANTS["RTGS_RANSAC_MAX_ITERS"]


def device_xyz(features: Dict, dev) -> torch.Tensor:
    """The features' "xyz" on the device, float64 [N, 3]: the host's array uploaded once and kept under "xyz_dev", so both forms
    hold the same bits."""
    hit = features.get("xyz_dev")
    if hit is None or hit.device != dev:
        hit = features["xyz_dev"] = torch.from_numpy(np.ascontiguousarray(features["xyz"], dtype=np.float64).reshape(-1, 3)).to(dev)
    return hit


def rigid_ransac_tables(matches, xyz, table, dev, max_hamming: int = 64, ratio: float = 0.8, iters: int = 512, inlier_dist: float = 0.05,
                        seed: int = 0) -> List[Dict]:
    """rtgs_rigid_ransac (include/rtgs_slam.h; the definition is tests/rigid_ransac_reference.py) for a batch of pairs: matches
    int32 [n, 3] and xyz float64 [m, 3] on the device `dev` (None for none), table [(first row and count nb of b's matches
    against a, first row and count na of a's against b, first row of a's points, first row of b's)] on the host.  -> per pair
    {"T" 4 x 4 float64, "n", "inliers", "rms", "h", "survivors", "ij" int32 [n, 2], "mask" bool [n]}; h = -1 (T and rms zero)
    without a valid hypothesis.  One launch and one copy to the host for the whole batch."""
    table = [tuple(int(v) for v in t) for t in table]
    if not table:
        return []
    if len(table) > 65535:
        raise ValueError("rigid_ransac_tables: at most 65535 pairs a launch")
    if not 1 <= int(iters) <= RANSAC_MAX_ITERS:
        raise ValueError(f"rigid_ransac_tables: iters must lie in 1 .. {RANSAC_MAX_ITERS}")
    for t, dtype, name in ((matches, torch.int32, "matches"), (xyz, torch.float64, "xyz")):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == dtype and t.dim() == 2
                                  and t.shape[1] == 3 and t.is_contiguous()):
            raise ValueError(f"rigid_ransac_tables: {name} must be a contiguous {dtype} [N, 3] tensor on the device")
    rows = min(RANSAC_CAP, max(0, max(t[1] for t in table)))
    rows += rows & 1
    out = torch.empty((len(table), RANSAC_HEAD + 3 * rows), dtype=torch.int32, device=dev)
    tab = torch.tensor(table, dtype=torch.int32).reshape(-1, 6).to(dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.rtgs_rigid_ransac(_lib.ptr0(matches), 0 if matches is None else int(matches.shape[0]), _lib.ptr0(xyz),
                                   0 if xyz is None else int(xyz.shape[0]), _lib.ptr(tab), len(table), int(max_hamming), float(ratio),
                                   int(iters), float(inlier_dist), int(seed) & 0xFFFFFFFF, rows, _lib.ptr(out), _lib.stream(dev))
    _lib.check(rc, "rtgs_rigid_ransac")
    host = out.cpu().numpy()                                                                      # the one copy
    f64 = np.ascontiguousarray(host[:, :34]).view(np.float64)
    res = []
    for p in range(len(table)):
        n = int(host[p, 34])
        m = host[p, RANSAC_HEAD:RANSAC_HEAD + 3 * n].reshape(n, 3)
        res.append({"T": f64[p, :16].reshape(4, 4).copy(), "n": n, "inliers": int(host[p, 35]), "rms": float(f64[p, 16]), "h": int(host[p, 36]),
                    "survivors": int(host[p, 37]), "ij": m[:, :2].copy(), "mask": m[:, 2] != 0})
    return res


def rigid_ransac_pairs(features, pairs: Sequence[Tuple], cfg=None, seed: int = 0, seconds: Dict = None) -> List[Dict]:
    """features: keyframe key -> detect_and_describe's dict; pairs: [(a, b)] -> per pair what pose_from_matches returns ("T" =
    T_a^-1 T_b with at least cfg.min_inliers witnesses, or None and a "reason"), plus "h", "ij" and "mask" of
    rigid_ransac_tables.  One match launch (both directions of every pair) and one rtgs_rigid_ransac launch for the whole batch,
    the match tables never leaving the device; one copy to the host.  The filter and the RANSAC are the definition's
    (tests/rigid_ransac_reference.py), which agrees with filter_matches and ransac_rigid in the matches and, to rounding, in
    the pose of one inlier set - not bit for bit.  With `seconds` (a dict) the device is synchronised behind the match launch and
    the dict gains "match" and "ransac", the seconds each took."""
    import time
    cfg = config() if cfg is None else cfg
    pairs = list(pairs)
    if not pairs:
        return []
    t0 = time.perf_counter()
    matches, where = match_pairs_device(features, [q for a, b in pairs for q in ((b, a), (a, b))])
    if seconds is not None:
        torch.cuda.synchronize(features[pairs[0][0]]["desc"].device)
        seconds["match"] = time.perf_counter() - t0
        t0 = time.perf_counter()
    keys = list(dict.fromkeys(k for pair in pairs for k in pair))   # in order of first appearance
    dev = features[keys[0]]["desc"].device
    begin, total = {}, 0
    for k in keys:
        begin[k] = total
        total += int(features[k]["desc"].shape[0])
    xyz = torch.cat([device_xyz(features[k], dev) for k in keys], dim=0).contiguous() if total else None
    table = [(where[2 * n][0], where[2 * n][1], where[2 * n + 1][0], where[2 * n + 1][1], begin[a], begin[b]) for n, (a, b) in enumerate(pairs)]
    fits = rigid_ransac_tables(matches, xyz, table, dev, cfg.max_hamming, cfg.ratio, cfg.ransac_iters, cfg.inlier_dist, seed)
    if seconds is not None:
        seconds["ransac"] = time.perf_counter() - t0
    res = []
    for (a, b), fit in zip(pairs, fits):
        out = {"T": None, "inliers": fit["inliers"], "matches": fit["n"], "rms": fit["rms"] if fit["h"] >= 0 else None,
               "keypoints_a": int(len(features[a]["x"])), "keypoints_b": int(len(features[b]["x"])), "reason": None,
               "h": fit["h"], "ij": fit["ij"], "mask": fit["mask"]}
        if out["inliers"] < cfg.min_inliers:
            out["reason"] = f"{out['inliers']} inliers of {fit['n']} matches, below {cfg.min_inliers}"
        else:
            out["T"] = fit["T"]
        res.append(out)
    return res


def keypoint_votes(matches, table, dev, max_hamming: int = 64, ratio: float = 0.8) -> torch.Tensor:
    """rtgs_keypoint_votes (include/rtgs_slam.h; the definition is tests/keypoint_pyramid_reference.votes): matches int32 [n, 3] on
    the device `dev` (None for none), table [(first row and count nb of b's matches against a, first row and count na of a's
    against b)] on the host -> int32 [pairs] on the device: per pair the rows that survive rigid_ransac_tables' filter, not
    capped.  One launch, nothing read."""
    table = np.asarray(table, dtype=np.int32).reshape(-1, 4)
    if matches is not None and not (torch.is_tensor(matches) and matches.is_cuda and matches.device == dev and matches.dtype == torch.int32
                                    and matches.dim() == 2 and matches.shape[1] == 3 and matches.is_contiguous()):
        raise ValueError("keypoint_votes: matches must be a contiguous int32 [N, 3] tensor on the device")
    votes = torch.zeros((len(table),), dtype=torch.int32, device=dev)
    if len(table) == 0:
        return votes
    tab = torch.from_numpy(table).to(dev)
    with torch.cuda.device(dev):
        rc = _lib.load().rtgs_keypoint_votes(_lib.ptr0(matches), 0 if matches is None else int(matches.shape[0]), _lib.ptr(tab), len(table),
                                             int(max_hamming), float(ratio), _lib.ptr(votes), _lib.stream(dev))
    _lib.check(rc, "rtgs_keypoint_votes")
    return votes


MAX_VOTE_PAIRS = 65535 // 2                                          # a match launch takes 65535 tables, a pair needs two


def vote_pairs(features, pairs: Sequence[Tuple], cfg=None) -> np.ndarray:
    """features: keyframe key -> detect_and_describe's dict; pairs: [(a, b)], at most MAX_VOTE_PAIRS -> int32 numpy [pairs]: how
    many matches of each pair survive the filter (mutual best, Hamming bound, ratio test).  One match launch (both directions of
    every pair) and one rtgs_keypoint_votes launch; the match tables stay on the device, only the counts are read."""
    cfg = config() if cfg is None else cfg
    pairs = list(pairs)
    if not pairs:
        return np.zeros((0,), dtype=np.int32)
    if len(pairs) > MAX_VOTE_PAIRS:
        raise ValueError(f"vote_pairs: at most {MAX_VOTE_PAIRS} pairs a launch")
    matches, where = match_pairs_device(features, [q for a, b in pairs for q in ((b, a), (a, b))])
    dev = features[pairs[0][0]]["desc"].device
    table = [(where[2 * n][0], where[2 * n][1], where[2 * n + 1][0], where[2 * n + 1][1]) for n in range(len(pairs))]
    return keypoint_votes(matches, table, dev, cfg.max_hamming, cfg.ratio).cpu().numpy()


def shortlist(votes, k: int, floor: int) -> List[int]:
    """votes[a] of one keyframe's partners a = 0 .. -> the up to k partners of the most votes that reach `floor`, a tie going to
    the lower index; in order of descending votes."""
    order = sorted((a for a, v in enumerate(votes) if v >= floor), key=lambda a: (-int(votes[a]), a))
    return order[:int(k)]
