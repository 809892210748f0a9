"""Host side of the RGB-D pose refinement (include/rtgs_icp.h, "RGB-D refinement"; csrc/rgbd_align.hip): a separate stage that
starts from the ICP tracker's answer and minimises point-to-plane distance AND intensity difference, so that a view whose
geometry does not constrain all six degrees of freedom (a wall seen head-on, a floor, a corridor) is still tracked where it has
texture.  Off by default (`rgbd_refine`); it touches none of the tracker's kernels.

    intensity_pyramid   colour [3,H,W] -> grey levels, coarsest first, the sizes of the ICP pyramids
    accumulate          one evaluation -> the 31 float64 sums on the device (two launches, no synchronisation)
    RgbdRefiner.refine  the Gauss-Newton loop: one host read of the 31 sums per iteration, the 6x6 solve on the host

tests/rgbd_align_reference.py is the definition: the sums match it bit for bit, the loop below is its numpy statement for
statement, so the refined pose does too.

With `rgbd_refine_exposure` (off by default; csrc/rgbd_exposure.hip, defined by tests/rgbd_exposure_reference.py) a gain and an
offset that take the source frame's intensity into the target's exposure are unknowns 7 and 8:

    accumulate_exposure       one evaluation -> the 48 float64 sums at (pose, alpha, beta)
    solve8                    the 8x8 solve on the host
    target_intensity_pyramid  the pyramid of a composite target: the map's rendered colour, and the frame's own - taken into
                              the map's exposure - where the model depth was filled from the frame

HIP tensors only."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib

OUT = _lib.CONSTANTS["RTGS_RGBD_ALIGN_OUT"]
OUT8 = _lib.CONSTANTS["RTGS_RGBD_EXPOSURE_OUT"]
NU, NH = 8, 36                   # unknowns with exposure on, entries of their upper triangle
ALPHA_MIN, ALPHA_MAX, BETA_MAX = 0.25, 4.0, 0.5
STOP = 1e-6
MIN_INLIERS = 6
RANK_TOL = 1e-9
DEFAULT_ITERS = (3, 3, 3)
DEFAULT_PHOTO_WEIGHT = 0.25      # metres per unit of intensity: 2 mm of depth noise at 1 m over 2 / 255 of intensity noise - derived,
DEFAULT_HUBER = 0.05             # not measured on real data; the Huber threshold (intensity units) is likewise a choice


def _require_device(t):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("rtg_slam_amd.rgbd_align: tensors must live on a HIP device; this build has no CPU path.")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


_vp, _stream = _lib.ptr, _lib.stream


def intensity_pyramid(color: torch.Tensor, levels: int = 3) -> List[torch.Tensor]:
    """colour [3,H,W] in 0..1 -> [H >> (L-1-l), W >> (L-1-l)] float32 for l = 0..L-1, coarsest first: grey =
    (0.299 R + 0.587 G) + 0.114 B, each coarser level the 2 x 2 mean of the next finer one (rtgs_rgbd_intensity_pyramid)."""
    lib = _lib.load()
    _require_device(color)
    if color.dim() != 3 or color.shape[0] != 3:
        raise ValueError("rtg_slam_amd.rgbd_align: colour must be [3,H,W]")
    dev = color.device
    color = _f32c(color)
    H, W = int(color.shape[1]), int(color.shape[2])
    levels = int(levels)
    if levels < 1 or (H >> (levels - 1)) < 1 or (W >> (levels - 1)) < 1:
        raise ValueError(f"rtg_slam_amd.rgbd_align: {levels} levels do not fit a {W}x{H} frame")
    out = [torch.empty(H >> (levels - 1 - l), W >> (levels - 1 - l), dtype=torch.float32, device=dev) for l in range(levels)]
    ptrs = (C.c_void_p * levels)(*[t.data_ptr() for t in out])
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_rgbd_intensity_pyramid(_vp(color), H, W, levels, ptrs, _stream(dev)), "rtgs_rgbd_intensity_pyramid")
    return out


def accumulate(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold: float, cos_threshold: float,
               photo_weight: float, huber: float, scratch: torch.Tensor | None = None) -> torch.Tensor:
    """rtgs_rgbd_align_accumulate -> the 31 float64 sums on the device, no synchronisation.  Maps [H,W,3] / [H,W] float32 of one
    level, K [3,3] of THAT level, pose [4,4] source -> target (both rounded to float32)."""
    lib = _lib.load()
    for t in (v_src, n_src, i_src, v_tgt, n_tgt, i_tgt):
        _require_device(t)
    dev = v_src.device
    H, W = int(v_src.shape[0]), int(v_src.shape[1])
    maps = [_f32c(t) for t in (v_src, n_src, i_src, v_tgt, n_tgt, i_tgt)]
    for t, last in zip(maps, ((3,), (3,), (), (3,), (3,), ())):
        if tuple(t.shape) != (H, W) + last or t.device != dev:
            raise ValueError("rtg_slam_amd.rgbd_align: vertex / normal maps must be [H,W,3] and intensity maps [H,W], one size, one device")
    K = _f32c(torch.as_tensor(K).to(dev)).reshape(-1)
    pose = _f32c(torch.as_tensor(pose).to(dev)).reshape(-1)
    if K.numel() != 9 or pose.numel() != 16:
        raise ValueError("rtg_slam_amd.rgbd_align: K must be 3x3 and pose 4x4")
    if scratch is None:
        scratch = torch.empty(max(lib.rtgs_rgbd_align_scratch_bytes(H, W) // 8, 1), dtype=torch.float64, device=dev)
    out = torch.empty(OUT, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.rtgs_rgbd_align_accumulate(*[_vp(t) for t in maps], H, W, _vp(K), _vp(pose), float(np.float32(distance_threshold)),
                                            float(np.float32(cos_threshold)), float(np.float32(photo_weight)),
                                            float(np.float32(huber)), _vp(out), _vp(scratch), _stream(dev))
    _lib.check(rc, "rtgs_rgbd_align_accumulate")
    return out


def _level_maps(maps, dev):
    H, W = int(maps[0].shape[0]), int(maps[0].shape[1])
    maps = [_f32c(t) for t in maps]
    for t, last in zip(maps, ((3,), (3,), (), (3,), (3,), ())):
        if tuple(t.shape) != (H, W) + last or t.device != dev:
            raise ValueError("rtg_slam_amd.rgbd_align: vertex / normal maps must be [H,W,3] and intensity maps [H,W], one size, one device")
    return H, W, maps


def accumulate_exposure(v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, pose, distance_threshold: float, cos_threshold: float,
                        photo_weight: float, huber: float, alpha: float, beta: float, scratch: torch.Tensor | None = None) -> torch.Tensor:
    """rtgs_rgbd_align_accumulate_exposure -> the 48 float64 sums on the device, no synchronisation.  The arguments of
    `accumulate`, and the gain and offset (rounded to float32) that take the source intensity into the target's exposure."""
    lib = _lib.load()
    for t in (v_src, n_src, i_src, v_tgt, n_tgt, i_tgt):
        _require_device(t)
    dev = v_src.device
    H, W, maps = _level_maps((v_src, n_src, i_src, v_tgt, n_tgt, i_tgt), dev)
    K = _f32c(torch.as_tensor(K).to(dev)).reshape(-1)
    pose = _f32c(torch.as_tensor(pose).to(dev)).reshape(-1)
    if K.numel() != 9 or pose.numel() != 16:
        raise ValueError("rtg_slam_amd.rgbd_align: K must be 3x3 and pose 4x4")
    if scratch is None:
        scratch = torch.empty(max(lib.rtgs_rgbd_align_exposure_scratch_bytes(H, W) // 8, 1), dtype=torch.float64, device=dev)
    out = torch.empty(OUT8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.rtgs_rgbd_align_accumulate_exposure(*[_vp(t) for t in maps], H, W, _vp(K), _vp(pose),
                                                     float(np.float32(distance_threshold)), float(np.float32(cos_threshold)),
                                                     float(np.float32(photo_weight)), float(np.float32(huber)),
                                                     float(np.float32(alpha)), float(np.float32(beta)), _vp(out), _vp(scratch),
                                                     _stream(dev))
    _lib.check(rc, "rtgs_rgbd_align_accumulate_exposure")
    return out


def _chw(color: torch.Tensor, H: int, W: int, what: str) -> torch.Tensor:
    if color.dim() == 3 and tuple(color.shape) == (H, W, 3):
        color = color.permute(2, 0, 1)
    elif color.dim() != 3 or tuple(color.shape) != (3, H, W):
        raise ValueError(f"rtg_slam_amd.rgbd_align: {what} must be [3,H,W] or [H,W,3] of the depth's size")
    return _f32c(color)


def target_intensity_pyramid(render_color, frame_color, depth_rendered, depth_filled, alpha: float, beta: float,
                             levels: int = 3) -> List[torch.Tensor]:
    """rtgs_rgbd_target_intensity: the intensity pyramid (coarsest first, the sizes of `intensity_pyramid`) of the composite
    target.  Where depth_filled != depth_rendered - the model's depth before and after icp.fill_model_depth, [H,W] or [H,W,1] -
    a pixel is alpha grey(frame_color) + beta, elsewhere grey(render_color); colours [3,H,W] or [H,W,3]."""
    lib = _lib.load()
    for t in (render_color, frame_color, depth_rendered, depth_filled):
        _require_device(t)
    dev = depth_rendered.device
    H, W = int(depth_rendered.shape[0]), int(depth_rendered.shape[1])
    dr, df = _f32c(depth_rendered), _f32c(depth_filled)
    if dr.numel() != H * W or df.numel() != H * W:
        raise ValueError("rtg_slam_amd.rgbd_align: the depth maps must be [H,W] or [H,W,1], one size")
    rc_, fc = _chw(render_color, H, W, "render_color"), _chw(frame_color, H, W, "frame_color")
    if any(t.device != dev for t in (rc_, fc, df)):
        raise ValueError("rtg_slam_amd.rgbd_align: one device")
    levels = int(levels)
    if levels < 1 or (H >> (levels - 1)) < 1 or (W >> (levels - 1)) < 1:
        raise ValueError(f"rtg_slam_amd.rgbd_align: {levels} levels do not fit a {W}x{H} frame")
    out = [torch.empty(H >> (levels - 1 - l), W >> (levels - 1 - l), dtype=torch.float32, device=dev) for l in range(levels)]
    ptrs = (C.c_void_p * levels)(*[t.data_ptr() for t in out])
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_rgbd_target_intensity(_vp(rc_), _vp(fc), _vp(dr), _vp(df), float(np.float32(alpha)),
                                                  float(np.float32(beta)), H, W, levels, ptrs, _stream(dev)),
                   "rtgs_rgbd_target_intensity")
    return out


def solve(out: np.ndarray, rank_tol: float = RANK_TOL) -> Tuple[np.ndarray, int]:
    """The sums -> (x, rank): H x = -b on the eigen-directions of H with lambda > rank_tol lambda_max, added in ascending order;
    what the view does not constrain stays at the initial guess."""
    A = np.zeros((6, 6), np.float64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = out[k]
            k += 1
    b = np.array(out[21:27], dtype=np.float64)
    lam, E = np.linalg.eigh(A)
    x, rank = np.zeros(6, np.float64), 0
    for j in range(6):
        if lam[j] > rank_tol * lam[5]:
            x = x - E[:, j] * (np.dot(E[:, j], b) / lam[j])
            rank += 1
    return x, rank


def solve8(out: np.ndarray, rank_tol: float = RANK_TOL) -> Tuple[np.ndarray, int]:
    """The 48 sums -> (x [8], rank): `solve` on the 8 x 8 matrix; x[6], x[7] are the steps of the gain and the offset."""
    A = np.zeros((NU, NU), np.float64)
    k = 0
    for i in range(NU):
        for j in range(i, NU):
            A[i, j] = A[j, i] = out[k]
            k += 1
    b = np.array(out[NH:NH + NU], dtype=np.float64)
    lam, E = np.linalg.eigh(A)
    x, rank = np.zeros(NU, np.float64), 0
    for j in range(NU):
        if lam[j] > rank_tol * lam[NU - 1]:
            x = x - E[:, j] * (np.dot(E[:, j], b) / lam[j])
            rank += 1
    return x, rank


def se3_exp(x) -> np.ndarray:
    """exp of the twist x = (w, v) -> 4x4 float64: rotation by Rodrigues, translation J_l v (the tracker's exp_se3)."""
    w, v = np.asarray(x[:3], dtype=np.float64), np.asarray(x[3:], dtype=np.float64)
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


def se3_log(T) -> np.ndarray:
    """The twist x = (w, v) with se3_exp(x) = T, float64, |w| <= pi: the inverse of `se3_exp` in its conventions (rotation
    first, translation = J_l v).  The axis comes from the skew part of R, and near pi from the symmetric part of R, where the skew
    part vanishes."""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])      # sin(th) axis
    sn = np.sqrt(np.dot(s, s))
    th = np.arctan2(sn, c)
    if th <= 1e-8:
        w = s                                                                         # sin(th) / th = 1 to rounding
    elif c > -0.99:
        w = s * (th / sn)
    else:
        B = ((R + R.T) / 2.0 - c * np.eye(3)) / (1.0 - c)                             # a a^T: (R + R^T) / 2 = cos I + (1 - cos) a a^T
        k = int(np.argmax(np.diag(B)))
        a = B[:, k] / np.sqrt(B[k, k])
        a = a / np.sqrt(np.dot(a, a))
        if np.dot(a, s) < 0:
            a = -a
        w = a * th
    Wh = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    W2 = Wh @ Wh
    I = np.eye(3)
    if th <= 1e-8:
        Jl = I
    else:
        Jl = I + Wh * ((1.0 - np.cos(th)) / (th * th)) + W2 * ((th - np.sin(th)) / (th * th * th))
    return np.concatenate([w, np.linalg.solve(Jl, t)])


def level_K(K, downscale) -> np.ndarray:
    Kl = np.asarray(K, dtype=np.float32).reshape(3, 3) * np.float32(downscale)
    Kl[2, 2] = np.float32(1)
    return Kl


class RgbdRefiner:
    """Reads, with getattr and a default: rgbd_refine_iters ([3, 3, 3], one count per pyramid level),
    rgbd_refine_photo_weight (0.25 m per unit of intensity), rgbd_refine_huber (0.05), rgbd_refine_exposure (False: with it
    `refine` also solves for the gain and offset between the two frames).  The gates are the ICP's own
    icp_distance_threshold and icp_normal_threshold (degrees)."""

    def __init__(self, args):
        self.iters = [int(i) for i in getattr(args, "rgbd_refine_iters", DEFAULT_ITERS)]
        self.photo_weight = float(getattr(args, "rgbd_refine_photo_weight", DEFAULT_PHOTO_WEIGHT))
        self.huber = float(getattr(args, "rgbd_refine_huber", DEFAULT_HUBER))
        self.exposure = bool(getattr(args, "rgbd_refine_exposure", False))
        self.distance_threshold = float(getattr(args, "icp_distance_threshold", 0.1))
        self.cos_threshold = float(np.cos(np.deg2rad(getattr(args, "icp_normal_threshold", 20.0))))
        if not self.iters or min(self.iters) < 0:
            raise ValueError("rgbd_refine_iters must be a non-empty list of non-negative counts")
        levels = getattr(args, "icp_downscales", None)
        if levels is not None and len(levels) != len(self.iters):
            raise ValueError(f"rgbd_refine_iters has {len(self.iters)} entries for {len(levels)} pyramid levels (icp_downscales)")
        if self.photo_weight < 0 or self.huber < 0:
            raise ValueError("rgbd_refine_photo_weight and rgbd_refine_huber must not be negative")
        self._scratch = {}

    def _scratch_for(self, H, W, dev, size_fn="rtgs_rgbd_align_scratch_bytes"):
        key = (H, W, dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream, size_fn)
        s = self._scratch.get(key)
        if s is None:
            s = torch.empty(max(getattr(_lib.load(), size_fn)(H, W) // 8, 1), dtype=torch.float64, device=dev)
            self._scratch[key] = s
        return s

    def refine(self, init_pose, v_src: Sequence[torch.Tensor], n_src, i_src, v_tgt, n_tgt, i_tgt, K, downscales,
               exposure=None) -> Tuple[np.ndarray, Dict]:
        """Pyramids coarsest first, K of the full-resolution frame, init_pose 4x4 source -> target.  -> (T [4,4] float64 on the
        host, report): "iterations" per level, "inliers_geometric" / "inliers_photometric" per evaluation, "rank" per solve,
        "rms_geometric_before" / "_after" and "rms_photometric_before" / "_after" (at the first and the last evaluation; the last
        precedes the last update), "reason", "host_reads" and "device_s" (the accumulation launches, by device events).
        With rgbd_refine_exposure the loop has eight unknowns and starts at `exposure` = (alpha, beta), default (1, 0); the
        report gains "exposure", the final pair, and "exposure_steps"."""
        if self.exposure:
            return self._refine_exposure(init_pose, v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, downscales,
                                         (1.0, 0.0) if exposure is None else exposure)
        _require_device(v_src[0])
        dev = v_src[0].device
        Kh = torch.as_tensor(K).detach().cpu().numpy()
        if len(self.iters) != len(downscales):
            raise ValueError(f"rgbd_refine_iters has {len(self.iters)} entries for {len(downscales)} pyramid levels")
        iters = self.iters
        T = np.array(init_pose, dtype=np.float64).reshape(4, 4)
        rep = {"iterations": [0] * len(downscales), "inliers_geometric": [], "inliers_photometric": [], "rank": [], "twists": [], "reason": "done"}
        first = last = None
        stop = False
        events = []
        for l, ds in enumerate(downscales):
            Kl = torch.from_numpy(level_K(Kh, ds)).to(dev)
            H, W = int(v_src[l].shape[0]), int(v_src[l].shape[1])
            scratch = self._scratch_for(H, W, dev)
            for _ in range(iters[l]):
                e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                pose = torch.from_numpy(T.astype(np.float32)).to(dev)
                e[0].record(torch.cuda.current_stream(dev))
                sums = accumulate(v_src[l], n_src[l], i_src[l], v_tgt[l], n_tgt[l], i_tgt[l], Kl, pose, self.distance_threshold,
                                  self.cos_threshold, self.photo_weight, self.huber, scratch)
                e[1].record(torch.cuda.current_stream(dev))
                events.append(e)
                out = sums.cpu().numpy()                          # the iteration's one host read
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
                x, rank = solve(out)
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
        rep["host_reads"] = len(events)
        rep["device_s"] = sum(a.elapsed_time(b) for a, b in events) * 1e-3
        return T, rep

    def _refine_exposure(self, init_pose, v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, downscales, exposure) -> Tuple[np.ndarray, Dict]:
        """tests/rgbd_exposure_reference.refine, statement for statement: the state is (T, alpha, beta) in float64 on the host."""
        _require_device(v_src[0])
        dev = v_src[0].device
        Kh = torch.as_tensor(K).detach().cpu().numpy()
        if len(self.iters) != len(downscales):
            raise ValueError(f"rgbd_refine_iters has {len(self.iters)} entries for {len(downscales)} pyramid levels")
        iters = self.iters
        T = np.array(init_pose, dtype=np.float64).reshape(4, 4)
        alpha, beta = np.float64(exposure[0]), np.float64(exposure[1])
        rep = {"iterations": [0] * len(downscales), "inliers_geometric": [], "inliers_photometric": [], "rank": [], "twists": [],
               "exposure_steps": [], "reason": "done"}
        first = last = None
        stop = False
        events = []
        for l, ds in enumerate(downscales):
            Kl = torch.from_numpy(level_K(Kh, ds)).to(dev)
            H, W = int(v_src[l].shape[0]), int(v_src[l].shape[1])
            scratch = self._scratch_for(H, W, dev, "rtgs_rgbd_align_exposure_scratch_bytes")
            for _ in range(iters[l]):
                e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                pose = torch.from_numpy(T.astype(np.float32)).to(dev)
                e[0].record(torch.cuda.current_stream(dev))
                sums = accumulate_exposure(v_src[l], n_src[l], i_src[l], v_tgt[l], n_tgt[l], i_tgt[l], Kl, pose,
                                           self.distance_threshold, self.cos_threshold, self.photo_weight, self.huber,
                                           np.float32(alpha), np.float32(beta), scratch)
                e[1].record(torch.cuda.current_stream(dev))
                events.append(e)
                out = sums.cpu().numpy()                          # the iteration's one host read
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
                x, rank = solve8(out)
                rep["rank"].append(rank)
                rep["twists"].append(x)
                if not (ALPHA_MIN <= alpha + x[6] <= ALPHA_MAX and abs(beta + x[7]) <= BETA_MAX):
                    rep["reason"], stop = "exposure out of range", True   # the pose stays where it was before this update
                    alpha, beta = np.float64(1.0), np.float64(0.0)
                    break
                T = se3_exp(x[:6]) @ T
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
        rep["host_reads"] = len(events)
        rep["device_s"] = sum(a.elapsed_time(b) for a, b in events) * 1e-3
        return T, rep
