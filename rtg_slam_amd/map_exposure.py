"""Host side of the mapper's exposure stage (include/rtgs_slam.h, "map exposure"; csrc/map_exposure.hip): every frame's colour is
brought into the MAP's exposure before any of it reaches the map, so that under auto-exposure the map's colour is one exposure
and not a patchwork.  Frame 0 defines the map's exposure.  Off by default (`map_exposure`); it touches none of the map-step kernels.

`Mapping.temp_points_init` renders the model at the new frame's tracked pose anyway.  Where that render and the frame agree in
depth they see the same surface, so their intensities differ by the frame's exposure relative to the map: a gain alpha and an
offset beta, fitted on the device by a Huber iteration followed by Huber iterations with a cut (tests/map_exposure_reference.py is
the definition, matched bit for bit).  The corrected colour clamp(alpha c + beta, 0, 1) goes into NEW tensors; the raw ones stay
what they were (the tracker and the evaluation hold them).

    MapExposure.fit      the iterations of one frame: two launches each, no host read
    MapExposure.apply    colour [3,H,W] -> ([3,H,W], [H,W,3]) in the map's exposure, one launch
    MapExposure.state    the device buffer: alpha, beta, the frame's start, code, accepted iterations, the last eight sums
    MapExposure.history  ONE host read when asked: per frame (alpha, beta, code, valid pixels, inliers)

`map_exposure_channels: rgb` (absent from every preset; absent or `grey` is everything above, unchanged) fits a gain and an offset
per colour channel instead, for a camera whose auto white balance lets the channels drift apart: the same schedule through
rtgs_white_balance_fit / _apply (include/rtgs_slam.h, "white balance"; csrc/white_balance.hip; tests/white_balance_reference.py),
source = the frame, target = the render, no bounds on the render's channels.  The grey regression runs beside the three channels;
a channel whose own regression is refused follows it.  `state` is then the RTGS_WHITE_BALANCE_STATE buffer and a history row
gains the three channels' (alpha, beta, code).

HIP tensors only."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib

STATE = _lib.CONSTANTS["RTGS_MAP_EXPOSURE_STATE"]
SUMS_AT = _lib.CONSTANTS["RTGS_MAP_EXPOSURE_SUMS_AT"]
WB_STATE = _lib.CONSTANTS["RTGS_WHITE_BALANCE_STATE"]
WB_REG = _lib.CONSTANTS["RTGS_WHITE_BALANCE_REG"]
WB_FRAME_AT = _lib.CONSTANTS["RTGS_WHITE_BALANCE_FRAME_AT"]
WB_SUMS_AT = _lib.CONSTANTS["RTGS_WHITE_BALANCE_SUMS_AT"]
WB_VALID = _lib.CONSTANTS["RTGS_WHITE_BALANCE_VALID"]
CHANNELS = ("grey", "rgb")
CODES = {0: "ok", 1: "too few valid pixels", 2: "no weight", 3: "no variance of intensity", 4: "not finite", 5: "out of range"}
# The Huber threshold is rgbd_refine_huber's; everything else is a choice, not a measurement
DEFAULTS = {"map_exposure_iters": 4, "map_exposure_huber": 0.05, "map_exposure_cut": 3.0, "map_exposure_depth_gate": 0.05,
            "map_exposure_t_gate": 0.1, "map_exposure_lo": 4.0 / 255.0, "map_exposure_hi": 251.0 / 255.0,
            "map_exposure_var_min": 1e-4, "map_exposure_min_valid": None}          # None: max(64, H W / 100)

_vp, _stream = _lib.ptr, _lib.stream


def refuse_pipeline(args) -> None:
    """For a caller that drives the mapper through rtg_slam_amd.pipeline.TrackMapPipeline: the stage is not built there."""
    if bool(getattr(args, "map_exposure", False)):
        raise ValueError("map_exposure is not built for rtg_slam_amd.pipeline (TrackMapPipeline): run it through slam.run_sequence")


def channels_of(args) -> str:
    """`map_exposure_channels` of a config: grey when absent."""
    ch = getattr(args, "map_exposure_channels", "grey")
    if ch not in CHANNELS:
        raise ValueError(f"map_exposure_channels must be one of {', '.join(CHANNELS)}, got {ch!r}")
    return ch


def white_balance_state(device) -> torch.Tensor:
    """A RTGS_WHITE_BALANCE_STATE buffer at identity: every regression (1, 0), started from (1, 0), no code."""
    st = torch.zeros(WB_STATE // WB_REG, WB_REG, dtype=torch.float64, device=device)
    st[:WB_FRAME_AT // WB_REG, 0] = 1.0
    st[:WB_FRAME_AT // WB_REG, 2] = 1.0
    return st.reshape(-1)


def white_balance_fit(lib, maps, H: int, W: int, iteration: int, gates, var_min: float, min_valid: int, state, scratch, device):
    """rtgs_white_balance_fit on the current stream: maps = (source colour, source depth, target colour, target depth, T_map),
    float32 and contiguous; gates = (huber, cut, depth_gate, t_gate, src_lo, src_hi, dst_lo, dst_hi)."""
    f = lambda x: float(np.float32(x))
    with torch.cuda.device(device):
        rc = lib.rtgs_white_balance_fit(*[_vp(t) for t in maps], H, W, int(iteration), *[f(x) for x in gates], float(var_min),
                                        int(min_valid), _vp(state), _vp(scratch), _stream(device))
    _lib.check(rc, "rtgs_white_balance_fit")


def min_valid_default(H: int, W: int) -> int:
    return max(64, (int(H) * int(W)) // 100)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


class MapExposure:
    """Reads, with getattr and the defaults above: map_exposure_iters (4: one Huber iteration, then three with the cut),
    map_exposure_huber, map_exposure_cut, map_exposure_depth_gate (m), map_exposure_t_gate, map_exposure_lo / _hi (the range of
    a channel that was not clamped), map_exposure_var_min, map_exposure_min_valid, map_exposure_channels (grey; rgb: a gain and an
    offset per colour channel)."""

    def __init__(self, args, device):
        g = lambda k: getattr(args, k, DEFAULTS[k])
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("rtg_slam_amd.map_exposure: needs a HIP device; this build has no CPU path.")
        self.iters = int(g("map_exposure_iters"))
        self.huber, self.cut = float(g("map_exposure_huber")), float(g("map_exposure_cut"))
        self.depth_gate, self.t_gate = float(g("map_exposure_depth_gate")), float(g("map_exposure_t_gate"))
        self.lo, self.hi = float(g("map_exposure_lo")), float(g("map_exposure_hi"))
        self.var_min = float(g("map_exposure_var_min"))
        mv = g("map_exposure_min_valid")
        self.min_valid = None if mv is None else int(mv)
        if self.iters < 1 or not self.huber > 0 or not self.cut >= 1 or not self.depth_gate >= 0 or not self.lo <= self.hi \
                or not self.var_min >= 0 or (self.min_valid is not None and self.min_valid < 1):
            raise ValueError("map_exposure: iters >= 1, huber > 0, cut >= 1, depth_gate >= 0, lo <= hi, var_min >= 0, min_valid >= 1")
        self.channels = channels_of(args)
        self.lib = _lib.load()
        if self.channels == "rgb":
            self.state = white_balance_state(self.device)
        else:
            self.state = torch.zeros(STATE, dtype=torch.float64, device=self.device)
            self.state[0] = 1.0
            self.state[2] = 1.0
        self._scratch = None
        self._hist: List = []                                    # per frame: a device copy of the state, None for an unfitted frame

    def options(self) -> Dict:
        """Every setting in force."""
        opts = {"iters": self.iters, "huber": self.huber, "cut": self.cut, "depth_gate": self.depth_gate, "t_gate": self.t_gate,
                "lo": self.lo, "hi": self.hi, "var_min": self.var_min, "min_valid": self.min_valid or "max(64, H W / 100)"}
        if self.channels == "rgb":
            opts["channels"] = "rgb"
        return opts

    def skip(self) -> None:
        """A frame with nothing to fit against (frame 0): nothing is launched, the state stays."""
        self._hist.append(None)

    def fit_iteration(self, frame_color_chw, frame_depth, render_color, render_depth, T_map, iteration: int) -> None:
        """rtgs_map_exposure_fit (rtgs_white_balance_fit with map_exposure_channels: rgb): one iteration on the current stream."""
        H, W = int(frame_color_chw.shape[-2]), int(frame_color_chw.shape[-1])
        maps = [_f32c(t) for t in (frame_color_chw, frame_depth, render_color, render_depth, T_map)]
        for t, k in zip(maps, (3, 1, 3, 1, 1)):
            if not t.is_cuda or t.device != self.device or t.numel() != k * H * W:
                raise ValueError("rtg_slam_amd.map_exposure: colours must be [3,H,W] and depths / T_map H W elements, on the stage's device")
        rgb = self.channels == "rgb"
        need = (self.lib.rtgs_white_balance_scratch_bytes if rgb else self.lib.rtgs_map_exposure_scratch_bytes)(H, W) // 8
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(max(need, 1), dtype=torch.float64, device=self.device)
        mv = self.min_valid if self.min_valid is not None else min_valid_default(H, W)
        if rgb:
            gates = (self.huber, self.cut, self.depth_gate, self.t_gate, self.lo, self.hi, float("-inf"), float("inf"))
            white_balance_fit(self.lib, maps, H, W, iteration, gates, self.var_min, mv, self.state, self._scratch, self.device)
            return
        f = lambda x: float(np.float32(x))
        with torch.cuda.device(self.device):
            rc = self.lib.rtgs_map_exposure_fit(*[_vp(t) for t in maps], H, W, int(iteration), f(self.huber), f(self.cut),
                                                f(self.depth_gate), f(self.t_gate), f(self.lo), f(self.hi), self.var_min, mv,
                                                _vp(self.state), _vp(self._scratch), _stream(self.device))
        _lib.check(rc, "rtgs_map_exposure_fit")

    def fit(self, frame_color_chw, frame_depth, render: Dict[str, torch.Tensor]) -> None:
        """One frame: `render` is the map at the frame's pose (Mapping._render: "render" [3,H,W], "depth", "T_map").  Starts from
        the previous frame's state; 2 launches per iteration, no synchronisation."""
        for k in range(self.iters):
            self.fit_iteration(frame_color_chw, frame_depth, render["render"], render["depth"], render["T_map"], k)
        self._hist.append(self.state.clone())

    def apply(self, color_chw: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """rtgs_map_exposure_apply (rtgs_white_balance_apply with map_exposure_channels: rgb) -> (chw, hwc): new tensors, the input
        is not written."""
        if color_chw.dim() != 3 or color_chw.shape[0] != 3 or not color_chw.is_cuda:
            raise ValueError("rtg_slam_amd.map_exposure: colour must be [3,H,W] on a HIP device")
        c = _f32c(color_chw)
        H, W = int(c.shape[1]), int(c.shape[2])
        chw = torch.empty(3, H, W, dtype=torch.float32, device=c.device)
        hwc = torch.empty(H, W, 3, dtype=torch.float32, device=c.device)
        name = "rtgs_white_balance_apply" if self.channels == "rgb" else "rtgs_map_exposure_apply"
        with torch.cuda.device(c.device):
            rc = getattr(self.lib, name)(_vp(c), H, W, _vp(self.state), _vp(chw), _vp(hwc), _stream(c.device))
        _lib.check(rc, name)
        return chw, hwc

    def history(self) -> List[Tuple]:
        """ONE host read: per frame (alpha, beta, code, valid pixels, inliers) as the frame's last iteration left them; a frame
        that was not fitted (frame 0) repeats the state it left alone, with code 0 and no pixels.  With map_exposure_channels: rgb
        these five are the grey regression's with the FRAME's code, followed by (alpha, beta, code) of red, green and blue."""
        rows = [h for h in self._hist if h is not None]
        host = torch.stack(rows).cpu().numpy() if rows else np.zeros((0, self.state.numel()))
        if self.channels == "rgb":
            out, j, last = [], 0, (1.0, 0.0) * 4
            for h in self._hist:
                if h is None:
                    out.append((last[0], last[1], 0, 0, 0) + tuple(x for c in (1, 2, 3) for x in (last[2 * c], last[2 * c + 1], 0)))
                    continue
                r = host[j]
                j += 1
                last = tuple(float(r[WB_REG * k + i]) for k in range(4) for i in (0, 1))
                out.append((last[0], last[1], int(r[WB_FRAME_AT]), int(r[WB_SUMS_AT + WB_VALID]), int(r[WB_SUMS_AT + 6]))
                           + tuple(x for c in (1, 2, 3) for x in (last[2 * c], last[2 * c + 1], int(r[WB_REG * c + 4]))))
            return out
        out, j, last = [], 0, (1.0, 0.0)
        for h in self._hist:
            if h is None:
                out.append((last[0], last[1], 0, 0, 0))
                continue
            r = host[j]
            j += 1
            last = (float(r[0]), float(r[1]))
            out.append((last[0], last[1], int(r[4]), int(r[SUMS_AT + 6]), int(r[SUMS_AT + 7])))
        return out

    def report(self) -> Dict:
        """What run_sequence puts under `map_exposure`."""
        hist = self.history()
        fitted = [(i, h) for i, h in enumerate(hist) if self._hist[i] is not None]
        al = [h[0] for _, h in fitted] or [1.0]
        be = [h[1] for _, h in fitted] or [0.0]
        fell = {str(i): CODES.get(h[2], str(h[2])) for i, h in fitted if h[2] != 0}
        rep = {"frames_fitted": len(fitted), "frames_fell_back": len(fell), "fell_back": fell,
               "alpha_mean": sum(al) / len(al), "alpha_min": min(al), "alpha_max": max(al),
               "beta_mean": sum(be) / len(be), "beta_min": min(be), "beta_max": max(be), "options": self.options()}
        if self.channels == "rgb":
            rep["channels"] = "rgb"
            for c, name in enumerate("rgb"):
                a = [h[5 + 3 * c] for _, h in fitted] or [1.0]
                b = [h[6 + 3 * c] for _, h in fitted] or [0.0]
                rep.update({f"alpha_{name}_mean": sum(a) / len(a), f"alpha_{name}_min": min(a), f"alpha_{name}_max": max(a),
                            f"beta_{name}_mean": sum(b) / len(b), f"beta_{name}_min": min(b), f"beta_{name}_max": max(b),
                            f"followed_grey_{name}": sum(1 for _, h in fitted if h[2] == 0 and h[7 + 3 * c] != 0)})
        return rep
