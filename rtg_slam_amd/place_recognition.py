"""Place recognition by appearance for the loop closure (csrc/place.hip; the definition is tests/place_reference.py).

    describe                    a keyframe's colour and depth -> its thumbnail descriptor (rtgs_place_describe), on the device
    score_pairs                 all pairs of descriptors at least min_gap apart -> score, shift, depth_rel (rtgs_place_scores)
    find_appearance_candidates  the pairs that look and measure alike (host, deterministic)
    appearance_init             the registration's starting pose from the best shift: a yaw, no translation

The small-image relocaliser of PTAM-style systems: a keyframe becomes a tw x th thumbnail of cell means; two keyframes are
compared by the zero-mean normalised cross-correlation of their grey thumbnails, searched over a horizontal shift of columns,
and by their depth thumbnails as a second witness.  ZNCC is blind to gain and offset.  Only yaw is searched; pitch, roll and
translation between the two views lower the score.  There is no fallback: a missing kernel is an error."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

SENTINEL_SCORE, SENTINEL_SHIFT, SENTINEL_DEPTH_REL = -2.0, 0, float("inf")
MAX_CELLS = _lib.CONSTANTS["RTGS_PLACE_MAX_CELLS"]
MAX_KEYFRAMES = _lib.CONSTANTS["RTGS_PLACE_MAX_KEYFRAMES"]


def thumb_height(H: int, W: int, tw: int) -> int:
    return max(1, round(tw * H / W))


def _check_image(color_chw, depth_chw):
    if not (torch.is_tensor(color_chw) and color_chw.is_cuda and color_chw.dtype == torch.float32 and color_chw.dim() == 3
            and color_chw.shape[0] == 3):
        raise ValueError("describe: colour must be a float32 [3, H, W] tensor on the device")
    H, W = int(color_chw.shape[1]), int(color_chw.shape[2])
    if not (torch.is_tensor(depth_chw) and depth_chw.device == color_chw.device and depth_chw.dtype == torch.float32
            and depth_chw.numel() == H * W):
        raise ValueError("describe: depth must be a float32 [1, H, W] tensor on the colour's device")
    return H, W


def describe(color_chw: torch.Tensor, depth_chw: torch.Tensor, tw: int = 40, out: Optional[Dict] = None, row: int = 0) -> Dict:
    """-> {"intensity", "depth", "valid"}: float32 [1, th, tw] on the device, th = thumb_height(H, W, tw).  With `out` (such a
    dict of [M, th, tw] arrays) the descriptor is written into its row `row` instead and `out` is returned."""
    H, W = _check_image(color_chw, depth_chw)
    tw = int(tw)
    th = thumb_height(H, W, tw) if tw >= 1 else 0
    if tw < 1 or tw > W or th > H or tw * th > MAX_CELLS:
        raise ValueError(f"describe: a thumbnail of width {tw} does not fit a {W} x {H} image (at most {MAX_CELLS} cells)")
    dev = color_chw.device
    if out is None:
        out = {k: torch.empty((1, th, tw), dtype=torch.float32, device=dev) for k in ("intensity", "depth", "valid")}
    for k in ("intensity", "depth", "valid"):
        t = out[k]
        if not (t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and t.dim() == 3 and tuple(t.shape[1:]) == (th, tw)
                and 0 <= int(row) < t.shape[0]):
            raise ValueError("describe: out must hold contiguous float32 [M, th, tw] arrays on the device, row inside them")
    color_chw, depth_chw = color_chw.contiguous(), depth_chw.contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.rtgs_place_describe(_lib.ptr(color_chw), _lib.ptr(depth_chw), H, W, tw, th, _lib.ptr(out["intensity"][int(row)]),
                                     _lib.ptr(out["depth"][int(row)]), _lib.ptr(out["valid"][int(row)]), _lib.stream(dev))
    _lib.check(rc, "rtgs_place_describe")
    return out


def describe_all(keymaps: Sequence[Dict], tw: int = 40) -> Dict:
    """The descriptors of a list of keyframe maps ({"color_chw", "depth_chw"}, as Mapping.keymap_list keeps them): [M, th, tw]."""
    if not keymaps:
        raise ValueError("describe_all: no keyframe")
    H, W = _check_image(keymaps[0]["color_chw"], keymaps[0]["depth_chw"])
    th = thumb_height(H, W, int(tw)) if int(tw) >= 1 else 0
    if int(tw) < 1 or int(tw) > W or th > H or int(tw) * th > MAX_CELLS:
        raise ValueError(f"describe: a thumbnail of width {tw} does not fit a {W} x {H} image (at most {MAX_CELLS} cells)")
    dev = keymaps[0]["color_chw"].device
    out = {k: torch.empty((len(keymaps), th, int(tw)), dtype=torch.float32, device=dev) for k in ("intensity", "depth", "valid")}
    for k, km in enumerate(keymaps):
        describe(km["color_chw"], km["depth_chw"], tw, out=out, row=k)
    return out


def score_pairs(desc: Dict, min_gap: int, max_shift: int = 4, rows: Optional[Tuple[int, int]] = None, out=None):
    """desc: {"intensity", "depth", "valid"} float32 [M, th, tw] on the device -> (score float32, shift int32, depth_rel
    float32), each [M, M] on the device and indexed [b, a].  Rows b in `rows` = (b_begin, b_end), default all, are computed;
    every other entry holds the sentinels -2, 0, +inf - or, with `out` (three such matrices), what it held."""
    I, D, V = desc["intensity"], desc["depth"], desc["valid"]
    for t in (I, D, V):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous()
                and t.shape == I.shape and t.device == I.device):
            raise ValueError("score_pairs: the descriptors must be contiguous float32 [M, th, tw] arrays on one device")
    M, th, tw = (int(x) for x in I.shape)
    S, min_gap = int(max_shift), int(min_gap)
    b0, b1 = (0, M) if rows is None else (int(rows[0]), int(rows[1]))
    if M < 1 or M > MAX_KEYFRAMES or tw * th > MAX_CELLS or S < 0 or 2 * S >= tw or min_gap < 1 or not 0 <= b0 <= b1 <= M:
        raise ValueError("score_pairs: 1 <= M <= %d, th tw <= %d, 0 <= 2 max_shift < tw, min_gap >= 1, 0 <= rows[0] <= rows[1] <= M"
                         % (MAX_KEYFRAMES, MAX_CELLS))
    dev = I.device
    if out is None:
        out = (torch.full((M, M), SENTINEL_SCORE, dtype=torch.float32, device=dev),
               torch.full((M, M), SENTINEL_SHIFT, dtype=torch.int32, device=dev),
               torch.full((M, M), SENTINEL_DEPTH_REL, dtype=torch.float32, device=dev))
    score, shift, rel = out
    for t, dt in ((score, torch.float32), (shift, torch.int32), (rel, torch.float32)):
        if not (t.dtype == dt and t.device == dev and t.is_contiguous() and tuple(t.shape) == (M, M)):
            raise ValueError("score_pairs: out must be contiguous [M, M] matrices (float32, int32, float32) on the device")
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.rtgs_place_scores(_lib.ptr(I), _lib.ptr(D), _lib.ptr(V), M, tw, th, S, min_gap, b0, b1, _lib.ptr(score),
                                   _lib.ptr(shift), _lib.ptr(rel), _lib.stream(dev))
    _lib.check(rc, "rtgs_place_scores")
    return score, shift, rel


def find_appearance_candidates(score, shift, depth_rel, min_gap: int, min_score: float = 0.9, max_depth_rel: float = 0.1,
                               max_per_keyframe: int = 2) -> List[Tuple[int, int, float, int, float]]:
    """The three matrices of score_pairs (tensors or arrays; they come to the host here, once) -> [(a, b, score, shift,
    depth_rel)] in ascending b: for keyframe b the a <= b - min_gap with score >= min_score and depth_rel <= max_depth_rel, best
    score first (ties: the lower depth_rel, then the older a), at most max_per_keyframe of them."""
    if int(min_gap) < 1 or int(max_per_keyframe) < 1:
        raise ValueError("find_appearance_candidates: min_gap and max_per_keyframe must be >= 1")
    if torch.is_tensor(score):
        host = torch.stack([score.to(torch.float64), shift.to(torch.float64), depth_rel.to(torch.float64)]).cpu().numpy()
        score, shift, depth_rel = host[0], host[1], host[2]
    score, shift, depth_rel = np.asarray(score), np.asarray(shift), np.asarray(depth_rel)
    out = []
    for b in range(score.shape[0]):
        hits = []
        for a in range(0, b - int(min_gap) + 1):
            sc, dr = float(score[b, a]), float(depth_rel[b, a])
            if sc >= min_score and dr <= max_depth_rel:
                hits.append((-sc, dr, a))
        hits.sort()
        out.extend((a, b, -msc, int(shift[b, a]), dr) for msc, dr, a in hits[:int(max_per_keyframe)])
    return out


def appearance_init(shift: int, fx: float, W: int, tw: int) -> np.ndarray:
    """4 x 4 float64, source (b) -> target (a) camera in register_pair's T_a^-1 T_b convention: a rotation about the camera's y
    axis by -atan(shift (W / tw) / fx) - a thumbnail column is W / tw pixels wide - and no translation."""
    th = -math.atan(shift * (W / tw) / fx)
    T = np.eye(4)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = math.cos(th), math.sin(th), -math.sin(th), math.cos(th)
    return T
