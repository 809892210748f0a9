"""Plain-numpy restatement of the white balance fit (include/rtgs_slam.h, "white balance"; csrc/white_balance.hip): a gain and an
offset per colour channel from a SOURCE picture to a TARGET picture, fitted on the pixels where the two see the same surface.  The
mapper calls it with source = frame, target = the map's render (map_exposure_channels: rgb); the exposure-aware evaluation with
source = the map's render, target = the frame.  Used only by tests; it is the definition the kernels are held to, bit for bit.
`weights`, `terms`, `solve`, the scenes and the defaults are tests/map_exposure_reference.py's, imported and unchanged.

    valid        every comparison in float32: source depth > 0, target depth > 0, |d_src - d_dst| <= depth_gate, T <= t_gate,
                 src_lo <= c <= src_hi for the three source channels, dst_lo <= c <= dst_hi for the three target channels, all six
                 finite.  A NaN fails every comparison; infinite bounds leave the "finite" test alone.
    regressions  k = 0: s = grey(source), t = grey(target), (0.299 r + 0.587 g) + 0.114 b as rgbd_align_reference forms it;
                 k = 1..3: s, t = the channel itself.  Each has its own (alpha_k, beta_k), its own float32 residual
                 r = to_target_exposure(s, alpha_k, beta_k) - t, its own weight (map_exposure_reference.weights) and seven float64
                 terms w, w s, w t, (w s) s, (w s) t, w (r r), (|r| <= huber ? 1 : 0); the valid pixel's 1 is accumulated once.
                 Row of a pixel: 7 k + j, the 1 at 28, three +0 up to 32.
    order        tests/mesh_register_reference.ordered_sum, unchanged, on the 32 columns.
    solve        map_exposure_reference.solve per regression on (S[7k .. 7k+5], valid, inliers): the same tests in the same order.
    frame rule   iteration 0 records every regression's (alpha, beta) as the frame's start and clears all codes.  Per iteration:
                 a channel that has a code keeps it and is not solved again; every other regression takes the code of its solve.
                 If the grey's code is not OK (too few valid pixels refuses all four) the frame's fit ends: all four regressions
                 return to the frame's start, the frame's code is the grey's, the remaining iterations change nothing (the sums
                 stay the refused iteration's).  Otherwise the grey is accepted, a channel whose code is OK is accepted, and a
                 channel with a code takes the grey's (alpha_0, beta_0) of THIS iteration: it follows the grey for the rest of the
                 frame.  (A channel without variance - a grey wall seen through one saturated channel - has no gain of its own to
                 fit, but it did see the exposure change the grey measured; leaving it at its start would tint the picture.)
    apply        per channel c = 1..3 to_target_exposure(c, alpha_c, beta_c), then fmin(fmax(., 0), 1) (a NaN becomes 0)."""
import numpy as np

from tests import map_exposure_reference as mer
from tests import mesh_register_reference as mrr
from tests.map_exposure_reference import (DEFAULTS, FLAT, NOT_FINITE, NO_WEIGHT, OK, RANGE, RECOVERY_CASES, ROBUST_SEEDS, TOO_FEW,
                                          exposed, min_valid_default, textured)
from tests.rgbd_align_reference import grey
from tests.rgbd_exposure_reference import to_target_exposure

F32, F64 = np.float32, np.float64
REGS, PER, VALID, OUT = 4, 7, 28, 32
INF = float("inf")
IDENTITY = ((1.0, 0.0),) * REGS


def valid_mask(src_color, src_depth, dst_color, dst_depth, T_map, depth_gate=DEFAULTS["depth_gate"], t_gate=DEFAULTS["t_gate"],
               src_lo=DEFAULTS["lo"], src_hi=DEFAULTS["hi"], dst_lo=-INF, dst_hi=INF):
    """-> [H,W] bool."""
    c = np.ascontiguousarray(src_color, dtype=F32)
    t = np.ascontiguousarray(dst_color, dtype=F32)
    H, W = c.shape[1:]
    d = np.ascontiguousarray(src_depth, dtype=F32).reshape(H, W)
    m = np.ascontiguousarray(dst_depth, dtype=F32).reshape(H, W)
    T = np.ascontiguousarray(T_map, dtype=F32).reshape(H, W)
    with np.errstate(all="ignore"):
        ok = (d > 0) & (m > 0) & (np.abs(d - m) <= F32(depth_gate)) & (T <= F32(t_gate))
        for k in range(3):
            ok &= (c[k] >= F32(src_lo)) & (c[k] <= F32(src_hi)) & np.isfinite(c[k])
            ok &= (t[k] >= F32(dst_lo)) & (t[k] <= F32(dst_hi)) & np.isfinite(t[k])
    return ok


def regressions(src_color, dst_color):
    """-> (s [4, N], t [4, N]) float32: the greys, then the three channels."""
    c = np.ascontiguousarray(src_color, dtype=F32)
    t = np.ascontiguousarray(dst_color, dtype=F32)
    s = np.stack([grey(c).reshape(-1)] + [c[k].reshape(-1) for k in range(3)])
    d = np.stack([grey(t).reshape(-1)] + [t[k].reshape(-1) for k in range(3)])
    assert s.dtype == F32 and d.dtype == F32
    return s, d


def rows(s, t, valid, ab, huber, cut, iteration, weight_fn=None):
    """-> [N, 32] float64: the row of every pixel, +0 rows for the invalid ones."""
    out = np.zeros((s.shape[1], OUT), F64)
    for k in range(REGS):
        e = mer.terms(s[k], t[k], valid, ab[k][0], ab[k][1], huber, cut, iteration, weight_fn)   # w, ws, wt, wss, wst, wrr, 1, in
        out[:, PER * k:PER * k + 6] = e[:, :6]
        out[:, PER * k + 6] = e[:, 7]
    out[:, VALID] = np.where(valid, 1.0, 0.0)
    return out


def solve(S, k, min_valid, var_min=DEFAULTS["var_min"]):
    """Regression k of the 32 sums -> (alpha, beta, code), as map_exposure_reference.solve."""
    return mer.solve(list(S[PER * k:PER * k + 6]) + [S[VALID], S[PER * k + 6]], min_valid, var_min)


def fit(src_color, src_depth, dst_color, dst_depth, T_map, state=IDENTITY, iters=DEFAULTS["iters"], huber=DEFAULTS["huber"],
        cut=DEFAULTS["cut"], depth_gate=DEFAULTS["depth_gate"], t_gate=DEFAULTS["t_gate"], src_lo=DEFAULTS["lo"],
        src_hi=DEFAULTS["hi"], dst_lo=-INF, dst_hi=INF, var_min=DEFAULTS["var_min"], min_valid=None, weight_fn=None):
    """One frame's fit from `state` (four (alpha, beta)) -> (ab [4][2] float64, codes [4], frame code, steps): steps[i] = dict(S,
    ab, codes, frame, iters) after iteration i, what the device buffer holds then."""
    H, W = np.asarray(src_color).shape[1:]
    min_valid = min_valid_default(H, W) if min_valid is None else min_valid
    valid = valid_mask(src_color, src_depth, dst_color, dst_depth, T_map, depth_gate, t_gate, src_lo, src_hi, dst_lo,
                       dst_hi).reshape(-1)
    s, t = regressions(src_color, dst_color)
    start = [(F64(a), F64(b)) for a, b in state]
    ab, codes, done, frame = list(start), [OK] * REGS, [0] * REGS, OK
    S, steps = np.zeros(OUT, F64), []
    for i in range(int(iters)):
        if frame == OK:
            S = mrr.ordered_sum(rows(s, t, valid, ab, huber, cut, i, weight_fn))
            a0, b0, frame = solve(S, 0, min_valid, var_min)
            codes[0] = frame
            new = list(start)
            if frame == OK:
                new[0] = (a0, b0)
                done[0] += 1
            for k in range(1, REGS):
                a, b = None, None
                if codes[k] == OK:
                    a, b, codes[k] = solve(S, k, min_valid, var_min)
                if frame != OK:
                    continue
                if codes[k] == OK:
                    new[k] = (a, b)
                    done[k] += 1
                else:
                    new[k] = new[0]
            ab = new
        steps.append(dict(S=S.copy(), ab=[(float(a), float(b)) for a, b in ab], codes=list(codes), frame=frame, iters=list(done)))
    return ab, codes, frame, steps


def state_vector(step, start=IDENTITY):
    """The RTGS_WHITE_BALANCE_STATE doubles of `step` for a frame that began at `start`."""
    v = np.zeros(72, F64)
    for k in range(REGS):
        v[8 * k:8 * k + 6] = (step["ab"][k][0], step["ab"][k][1], start[k][0], start[k][1], step["codes"][k], step["iters"][k])
    v[32] = step["frame"]
    v[40:72] = step["S"]
    return v


def apply(color, ab):
    """colour [3,H,W], ab = the four (alpha, beta) -> ([3,H,W], [H,W,3]) float32; the grey pair is not used."""
    c = np.ascontiguousarray(color, dtype=F32)
    with np.errstate(all="ignore"):
        out = np.stack([np.fmin(np.fmax(to_target_exposure(c[k], ab[k + 1][0], ab[k + 1][1]), F32(0)), F32(1)) for k in range(3)])
    assert out.dtype == F32
    return out, np.ascontiguousarray(out.transpose(1, 2, 0))


# ---- the scenes the CPU and GPU tests share ----

def tinted(clean, gains, offsets):
    """What a camera with auto white balance delivers of `clean`: channel k at (gains[k], offsets[k]), clamped as `exposed`."""
    clean = np.asarray(clean, F32)
    return np.stack([exposed(clean[k], gains[k], offsets[k]) for k in range(3)])


def channel_cases(k):
    """Three DIFFERENT (gain, offset) pairs of RECOVERY_CASES for the three channels: k, k + 1, k + 2 (mod 5)."""
    n = len(RECOVERY_CASES)
    return [RECOVERY_CASES[(k + j) % n] for j in range(3)]


def scene(H=60, W=80, gains=(1.0, 1.0, 1.0), offsets=(0.0, 0.0, 0.0), outliers=0.0, seed=0, clean=None):
    """map_exposure_reference.scene with a tinted frame: source = the frame, target = a render of `clean`."""
    clean = textured(H, W) if clean is None else clean
    frame = tinted(clean, gains, offsets)
    if outliers > 0:
        rng = np.random.default_rng(seed)
        hit = rng.random((H, W)) < outliers
        frame = np.where(hit[None], rng.uniform(0.05, 0.95, (3, H, W)).astype(F32), frame)
    d = np.full((H, W), 2.0, F32)
    return dict(src_color=frame, src_depth=d, dst_color=clean.copy(), dst_depth=d.copy(), T_map=np.zeros((H, W), F32))


def constant_channel_scene(H=60, W=80, channel=2, value=0.5, gains=(1.25, 0.8, 1.0), offsets=(-0.06, 0.08, 0.0)):
    """`scene` whose clean colour is constant in one channel: that channel's regression has no variance (code 3) and follows the grey."""
    clean = textured(H, W)
    clean[channel] = F32(value)
    return scene(H, W, gains, offsets, clean=clean)


def gated_scene(H=60, W=80, gains=(1.2, 0.9, 1.1), offsets=(-0.03, 0.04, 0.0), seed=0):
    """map_exposure_reference.gated_scene's gates on a tinted frame, plus target channels outside 4/255 .. 251/255 (they fail only
    under finite dst bounds)."""
    g = mer.gated_scene(H, W, seed=seed)
    frame = tinted(textured(H, W), gains, offsets)
    keep = (g["frame_color"] == 0) | (g["frame_color"] == 1)                   # the clamped channels of the grey scene
    s = dict(src_color=np.where(keep, g["frame_color"], frame).astype(F32), src_depth=g["frame_depth"], dst_color=g["render_color"],
             dst_depth=g["render_depth"], T_map=g["T_map"])
    if H * W > 1:
        rng = np.random.default_rng(200 + seed)
        hit = rng.random((H, W)) < 0.03
        s["dst_color"][0][hit] = 1.0
    return s


def as_grey(s):
    """A scene of this module under the argument names of map_exposure_reference.fit."""
    return dict(frame_color=s["src_color"], frame_depth=s["src_depth"], render_color=s["dst_color"], render_depth=s["dst_depth"],
                T_map=s["T_map"])
