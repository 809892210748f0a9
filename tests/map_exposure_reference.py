"""Plain-numpy restatement of the mapper's exposure stage (include/rtgs_slam.h, "map exposure"; csrc/map_exposure.hip;
rtg_slam_amd/map_exposure.py): a gain `alpha` and an offset `beta` per frame that take the frame's colour into the MAP's exposure
(frame 0 defines it), fitted on the pixels where the frame and the map rendered at the frame's pose see the same surface.  Used
only by tests; it is the definition the kernels are held to, bit for bit.  `grey` is rgbd_align_reference's and the two-step
`to_target_exposure` rgbd_exposure_reference's, imported and unchanged.

    valid    every comparison in float32: frame depth > 0, render depth > 0, |d_frame - d_render| <= depth_gate, T <= t_gate,
             lo <= c <= hi for the three frame channels (a channel the sensor or the stream clamped obeys no affine law), the
             three render channels finite.  A NaN fails every comparison.
    pixel    I = grey(frame), R = grey(render); Ic = to_target_exposure(I, alpha, beta) with the float64 state rounded to
             float32; r = Ic - R, a = |r| (float32).  w (float32) = 1 when a <= huber, else huber / a; from iteration 1 on also
             0 where a > cut huber (the product rounded to float32).  Iteration 0 is plain Huber because a weight that redescends
             diverges from a start 25 % of gain away (tests/test_map_exposure_cpu.py asserts it).
    terms    float64 on the widened float32 values: w, w I, w R, (w I) I, (w I) R, w (r r), 1, (a <= huber ? 1 : 0); an invalid
             pixel contributes +0 to all eight.
    order    tests/mesh_register_reference.ordered_sum, unchanged: chunks of 1024 pixels in row-major order, 256 slots of four
             strided pixels, `tree`, the chunk sums by slot chunk % 256, `tree`.
    solve    float64, one rounded operation each: det = S0 S3 - S1 S1, alpha = (S0 S4 - S1 S2) / det, beta = (S2 - alpha S1) / S0.
    accept   in this order, the first that fails gives the code: S6 >= min_valid (TOO_FEW), S0 > 0 (NO_WEIGHT),
             det > var_min (S0 S0) (FLAT), alpha and beta finite (NOT_FINITE), 0.25 <= alpha <= 4 and |beta| <= 0.5 (RANGE, the
             tracker's limits).  A rejected iteration ends the frame's fit: the state returns to what it was when the frame
             began, the code is kept, the remaining iterations change nothing (the sums stay the rejected iteration's).
    apply    per channel to_target_exposure(c, alpha, beta), then fmin(fmax(., 0), 1) (a NaN becomes 0)."""
import numpy as np

from tests import mesh_register_reference as mrr
from tests.rgbd_align_reference import grey
from tests.rgbd_exposure_reference import ALPHA_MAX, ALPHA_MIN, BETA_MAX, to_target_exposure

F32, F64 = np.float32, np.float64
OUT = 8
OK, TOO_FEW, NO_WEIGHT, FLAT, NOT_FINITE, RANGE = 0, 1, 2, 3, 4, 5
DEFAULTS = dict(iters=4, huber=0.05, cut=3.0, depth_gate=0.05, t_gate=0.1, lo=4.0 / 255.0, hi=251.0 / 255.0, var_min=1e-4)


def min_valid_default(H, W):
    return max(64, (int(H) * int(W)) // 100)


def valid_mask(frame_color, frame_depth, render_color, render_depth, T_map, depth_gate=DEFAULTS["depth_gate"],
               t_gate=DEFAULTS["t_gate"], lo=DEFAULTS["lo"], hi=DEFAULTS["hi"]):
    """-> [H,W] bool."""
    c = np.ascontiguousarray(frame_color, dtype=F32)
    rc = np.ascontiguousarray(render_color, dtype=F32)
    H, W = c.shape[1:]
    d = np.ascontiguousarray(frame_depth, dtype=F32).reshape(H, W)
    rd = np.ascontiguousarray(render_depth, dtype=F32).reshape(H, W)
    T = np.ascontiguousarray(T_map, dtype=F32).reshape(H, W)
    with np.errstate(all="ignore"):
        ok = (d > 0) & (rd > 0) & (np.abs(d - rd) <= F32(depth_gate)) & (T <= F32(t_gate))
        for k in range(3):
            ok &= (c[k] >= F32(lo)) & (c[k] <= F32(hi)) & np.isfinite(rc[k])
    return ok


def weights(a, huber, cut, iteration):
    """|r| [.] float32 -> w float32."""
    h = F32(huber)
    with np.errstate(all="ignore"):
        w = np.where(a <= h, F32(1), h / a)
        if iteration >= 1:
            w = np.where(a > F32(cut) * h, F32(0), w)
    assert w.dtype == F32
    return w


def terms(I, R, valid, alpha, beta, huber, cut, iteration, weight_fn=None):
    """I, R [N] float32, valid [N] bool -> [N, 8] float64."""
    with np.errstate(all="ignore"):
        r = to_target_exposure(I, alpha, beta) - R
        a = np.abs(r)
        w = (weight_fn or weights)(a, huber, cut, iteration)
        assert r.dtype == F32 and w.dtype == F32
        wd, Id, Rd, rd = (x.astype(F64) for x in (w, I, R, r))
        wI = wd * Id
        t = np.stack([wd, wI, wd * Rd, wI * Id, wI * Rd, wd * (rd * rd), np.ones_like(wd), (a <= F32(huber)).astype(F64)], axis=1)
    return np.where(valid[:, None], t, 0.0)


def solve(S, min_valid, var_min=DEFAULTS["var_min"]):
    """The eight sums -> (alpha, beta, code); alpha, beta are None unless the code is OK."""
    S = [F64(x) for x in S]
    if not S[6] >= F64(min_valid):
        return None, None, TOO_FEW
    if not S[0] > 0:
        return None, None, NO_WEIGHT
    with np.errstate(all="ignore"):
        det = S[0] * S[3] - S[1] * S[1]
        if not det > F64(var_min) * (S[0] * S[0]):
            return None, None, FLAT
        alpha = (S[0] * S[4] - S[1] * S[2]) / det
        beta = (S[2] - alpha * S[1]) / S[0]
    if not (np.isfinite(alpha) and np.isfinite(beta)):
        return None, None, NOT_FINITE
    if not (ALPHA_MIN <= alpha <= ALPHA_MAX and abs(beta) <= BETA_MAX):
        return None, None, RANGE
    return alpha, beta, OK


def fit(frame_color, frame_depth, render_color, render_depth, T_map, state=(1.0, 0.0), iters=DEFAULTS["iters"],
        huber=DEFAULTS["huber"], cut=DEFAULTS["cut"], depth_gate=DEFAULTS["depth_gate"], t_gate=DEFAULTS["t_gate"],
        lo=DEFAULTS["lo"], hi=DEFAULTS["hi"], var_min=DEFAULTS["var_min"], min_valid=None, weight_fn=None):
    """One frame's fit from `state` -> ((alpha, beta) float64, code, steps): steps[k] = (the eight sums, alpha, beta, code) after
    iteration k, what the device buffer holds then."""
    H, W = np.asarray(frame_color).shape[1:]
    min_valid = min_valid_default(H, W) if min_valid is None else min_valid
    valid = valid_mask(frame_color, frame_depth, render_color, render_depth, T_map, depth_gate, t_gate, lo, hi).reshape(-1)
    I, R = grey(frame_color).reshape(-1), grey(render_color).reshape(-1)
    start = (F64(state[0]), F64(state[1]))
    alpha, beta = start
    code, S, steps = OK, np.zeros(OUT, F64), []
    for k in range(int(iters)):
        if code == OK:
            S = mrr.ordered_sum(terms(I, R, valid, alpha, beta, huber, cut, k, weight_fn))
            a, b, code = solve(S, min_valid, var_min)
            alpha, beta = (a, b) if code == OK else start
        steps.append((S.copy(), float(alpha), float(beta), code))
    return (alpha, beta), code, steps


def apply(color, alpha, beta):
    """colour [3,H,W] -> ([3,H,W], [H,W,3]) float32 in the map's exposure."""
    with np.errstate(all="ignore"):
        out = np.fmin(np.fmax(to_target_exposure(color, alpha, beta), F32(0)), F32(1))
    assert out.dtype == F32
    return out, np.ascontiguousarray(out.transpose(1, 2, 0))


# ---- the scenes the CPU and GPU tests share ----

RECOVERY_CASES = ((1.0, 0.0), (1.25, -0.06), (0.8, 0.08), (1.25, 0.08), (0.8, -0.08))      # (gain, offset) of the frame
ROBUST_SEEDS = (0, 1, 2, 3, 4)


def textured(H=60, W=80, c=0.0, lo=0.5, amp=0.35):
    """The clean colour [3,H,W]: lo + amp sin(x / 5 + c) cos(y / 7), the three channels at phases c, c + 0.4, c + 0.8."""
    x, y = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64))
    return np.stack([lo + amp * np.sin(x / 5 + c + 0.4 * k) * np.cos(y / 7) for k in range(3)]).astype(F32)


def exposed(clean, gain, offset):
    """What the camera delivers of `clean` at (gain, offset): clamp(gain clean + offset, 0, 1)."""
    return np.clip(F32(gain) * np.asarray(clean, F32) + F32(offset), F32(0), F32(1)).astype(F32)


def scene(H=60, W=80, gain=1.0, offset=0.0, outliers=0.0, seed=0, clean=None):
    """A frame of `clean` at (gain, offset) over a render of `clean`, both at depth 2, T = 0; `outliers` of the frame's pixels
    get a random colour in [0.05, 0.95].  -> dict(frame_color, frame_depth, render_color, render_depth, T_map)."""
    clean = textured(H, W) if clean is None else clean
    frame = exposed(clean, gain, offset)
    if outliers > 0:
        rng = np.random.default_rng(seed)
        hit = rng.random((H, W)) < outliers
        frame = np.where(hit[None], rng.uniform(0.05, 0.95, (3, H, W)).astype(F32), frame)
    d = np.full((H, W), 2.0, F32)
    return dict(frame_color=frame, frame_depth=d, render_color=clean.copy(), render_depth=d.copy(), T_map=np.zeros((H, W), F32))


def gated_scene(H=60, W=80, gain=1.2, offset=-0.03, seed=0):
    """`scene` with every gate exercised: holes in either depth, depth disagreements, transparent pixels, clamped channels and
    non-finite render channels, each on its own pixels."""
    s = scene(H, W, gain, offset)
    rng = np.random.default_rng(100 + seed)
    pick = rng.integers(0, 8, (H, W)) if H * W > 1 else np.zeros((H, W), np.int64)
    u = rng.random((H, W)).astype(F32)
    hit = u < 0.3
    s["frame_depth"][hit & (pick == 1)] = 0.0
    s["render_depth"][hit & (pick == 2)] = 0.0
    s["render_depth"][hit & (pick == 3)] += F32(0.08)
    s["T_map"][hit & (pick == 4)] = 0.5
    s["frame_color"][0][hit & (pick == 5)] = 1.0
    s["frame_color"][2][hit & (pick == 6)] = 0.0
    s["render_color"][1][hit & (pick == 7)] = np.nan
    return s
