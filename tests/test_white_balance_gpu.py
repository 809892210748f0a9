"""csrc/white_balance.hip and the rgb mode of rtg_slam_amd/map_exposure.py against their definition,
tests/white_balance_reference.py: the 32 float64 sums and the whole state bit for bit after every iteration - also where a slot of
the second launch adds more than one chunk value - regression 0 against the existing grey kernels, the corrected colour in both
layouts, and the mapper on a short sequence whose frames change white balance."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import map_exposure_reference as mer
from tests import test_map_exposure_gpu as grey_gpu
from tests import white_balance_reference as wbr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
NAMES = ("src_color", "src_depth", "dst_color", "dst_depth", "T_map")
WB_ENTRIES = ("rtgs_white_balance_fit", "rtgs_white_balance_apply", "rtgs_white_balance_scratch_bytes")
# the grey test's sizes, and 257 chunks: the smallest picture at which a slot of the second launch (slot 0) adds more than one
# chunk value and the last chunk is partly empty (513 x 512 = 256 x 1024 + 512)
SIZES = grey_gpu.SIZES + [(513, 512)]
START = ((0.8, 0.05), (1.1, -0.02), (0.9, 0.0), (1.0, 0.03))
# how the two callers gate: the mapper bounds the source (the frame), the evaluation the target (the frame)
MODES = {"mapper": dict(src_lo=4 / 255, src_hi=251 / 255, dst_lo=-np.inf, dst_hi=np.inf),
         "evaluation": dict(src_lo=-np.inf, src_hi=np.inf, dst_lo=4 / 255, dst_hi=251 / 255)}
dev, bits, bits32 = grey_gpu.dev, grey_gpu.bits, grey_gpu.bits32


def run(s, start=wbr.IDENTITY, iters=4, huber=0.05, cut=3.0, depth_gate=0.05, t_gate=0.1, src_lo=4 / 255, src_hi=251 / 255,
        dst_lo=-np.inf, dst_hi=np.inf, var_min=1e-4, min_valid=None):
    """The kernels, one iteration at a time -> the host copy of the state after each."""
    from rtg_slam_amd import _lib, map_exposure as me
    lib = _lib.load()
    H, W = s["src_color"].shape[1:]
    state = me.white_balance_state(DEV)
    for k, (a, b) in enumerate(start):
        state[8 * k], state[8 * k + 1] = a, b
    d = [dev(s[k]) for k in NAMES]
    scratch = torch.empty(lib.rtgs_white_balance_scratch_bytes(H, W) // 8, dtype=torch.float64, device=DEV)
    mv = mer.min_valid_default(H, W) if min_valid is None else min_valid
    out = []
    for k in range(iters):
        me.white_balance_fit(lib, d, H, W, k, (huber, cut, depth_gate, t_gate, src_lo, src_hi, dst_lo, dst_hi), var_min, mv, state,
                             scratch, DEV)
        out.append(state.cpu().numpy().copy())
    return out


def assert_matches(states, steps, start):
    assert len(states) == len(steps)
    for k, (st, step) in enumerate(zip(states, steps)):
        want = wbr.state_vector(step, start)
        assert np.array_equal(bits(st[40:72]), bits(want[40:72])), (k, st[40:72], want[40:72])
        assert np.array_equal(bits(st), bits(want)), (k, st[:40], want[:40])


@functools.lru_cache(maxsize=None)
def mapper_case(H, W):
    """(scene, kernels' states, the definition's steps, overrides) at the mapper's gates from START: computed once per size."""
    s = wbr.gated_scene(H, W)
    over = {"min_valid": 1} if H * W == 1 else {}
    return s, run(s, START, **over), wbr.fit(**s, state=START, **over), over


@pytest.mark.parametrize("H,W", SIZES)
def test_sums_and_state_match_the_definition_after_every_iteration(H, W):
    s, states, (ab, codes, frame, steps), _ = mapper_case(H, W)
    assert_matches(states, steps, START)
    if H * W == 1:                                                              # one pixel has no variance; by default it is too few
        assert frame == wbr.FLAT
        states = run(s, START)
        _, _, frame, steps = wbr.fit(**s, state=START)
        assert frame == wbr.TOO_FEW
        assert_matches(states, steps, START)
    else:
        assert frame == wbr.OK and codes == [wbr.OK] * 4
        assert states[-1][40 + wbr.VALID] > 0.5 * H * W and not states[-1][69:72].any()


@pytest.mark.parametrize("H,W", [(60, 80), (25, 41), (513, 512)])
def test_the_evaluation_gates_match_the_definition(H, W):
    s = wbr.gated_scene(H, W)
    states = run(s, **MODES["evaluation"])
    _, _, frame, steps = wbr.fit(**s, **MODES["evaluation"])
    assert_matches(states, steps, wbr.IDENTITY)
    assert frame == wbr.OK
    valid = wbr.valid_mask(**s, **MODES["evaluation"]).sum()
    assert states[-1][40 + wbr.VALID] == valid != wbr.valid_mask(**s).sum()      # the two callers gate different pixels


@pytest.mark.parametrize("H,W", SIZES)
def test_regression_0_is_the_grey_kernel(H, W):
    """With infinite dst bounds: the six sums, the inlier count, the valid count and (alpha_0, beta_0) are what
    rtgs_map_exposure_fit leaves for the same inputs, bit for bit, after every iteration."""
    s, states, _, over = mapper_case(H, W)
    grey = grey_gpu.run(wbr.as_grey(s), START[0], **over)
    for k, (st, g) in enumerate(zip(states, grey)):
        assert np.array_equal(bits(st[40:46]), bits(g[8:14])), k
        assert bits(st[46]) == bits(g[15]) and bits(st[40 + wbr.VALID]) == bits(g[14]), k
        assert np.array_equal(bits(st[0:2]), bits(g[0:2])), k
        assert st[32] == g[4] == st[4]


def test_frame_rule_through_the_kernels():
    s = wbr.constant_channel_scene(channel=2)
    states = run(s, START)
    ab, codes, frame, steps = wbr.fit(**s, state=START)
    assert_matches(states, steps, START)
    assert frame == wbr.OK and codes == [0, 0, 0, wbr.FLAT]
    for st in states:
        assert st[32] == 0 and st[28] == wbr.FLAT and np.array_equal(bits(st[24:26]), bits(st[0:2]))
    assert list(states[-1][[5, 13, 21, 29]]) == [4, 4, 4, 0]
    few = wbr.scene(gains=(1.25, 0.8, 1.0), offsets=(-0.06, 0.08, 0.0))
    few["src_depth"][:, 1:] = 0
    grey_flat = wbr.scene(clean=np.full((3, 60, 80), 0.5, F32))
    grey_range = wbr.scene(gains=(5.0, 5.0, 1.0), clean=mer.textured(lo=0.1, amp=0.07))
    for sc, want in ((few, wbr.TOO_FEW), (grey_flat, wbr.FLAT), (grey_range, wbr.RANGE)):
        states = run(sc, START)
        _, _, frame, steps = wbr.fit(**sc, state=START)
        assert_matches(states, steps, START)
        assert frame == want
        for st in states:                                                       # all four are back at the frame's start
            assert st[32] == want and [tuple(st[8 * k:8 * k + 2]) for k in range(4)] == list(START)
            assert np.array_equal(bits(st[40:72]), bits(states[0][40:72]))


@pytest.mark.parametrize("k", range(len(mer.RECOVERY_CASES)))
def test_recovery_through_the_kernels(k):
    from tests import test_white_balance_cpu as cpu
    cs, s = cpu.tinted_scene(k)
    states = run(s)
    _, _, frame, steps = wbr.fit(**s)
    assert_matches(states, steps, wbr.IDENTITY)
    assert frame == wbr.OK
    for j in range(3):
        assert cpu.off(states[-1][8 * (j + 1):8 * (j + 1) + 2], *cs[j]) <= cpu.recovery_bound()


def test_two_runs_are_bit_equal_and_refusals_launch_nothing():
    from rtg_slam_amd import _lib, map_exposure as me
    s = wbr.gated_scene(60, 80)
    a, b = run(s, START), run(s, START)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
    lib = _lib.load()
    for H, W in SIZES + [(680, 1200)]:
        assert lib.rtgs_white_balance_scratch_bytes(H, W) == -(-H * W // 1024) * 32 * 8
    for H, W in ((0, 80), (60, 0), (-1, 80), (65536, 65536), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.rtgs_white_balance_scratch_bytes(H, W) == 0
    E = _lib.CONSTANTS["RTGS_E_INVALID"]
    state = me.white_balance_state(DEV)
    state[8], state[9] = 0.7, 0.1
    before = state.clone()
    d = [dev(s[k]) for k in NAMES]
    scratch = torch.empty(lib.rtgs_white_balance_scratch_bytes(60, 80) // 8, dtype=torch.float64, device=DEV)
    out = torch.empty(2, 3 * 60 * 80, dtype=torch.float32, device=DEV)
    p, st = _lib.ptr, _lib.stream(DEV)
    inf, nan = float("inf"), float("nan")
    #                     5   6   7  8     9    10    11   12       13         14    15   16    17  18        19          20
    good = [p(t) for t in d] + [60, 80, 0, 0.05, 3.0, 0.05, 0.1, 4 / 255, 251 / 255, -inf, inf, 1e-4, 64, p(state), p(scratch), st]
    for i in (0, 1, 2, 3, 4, 18, 19):                                           # a null pointer
        bad = list(good)
        bad[i] = None
        assert lib.rtgs_white_balance_fit(*bad) == E, i
    for i, v in ((5, 0), (6, 0), (5, 65536), (7, -1), (8, 0.0), (8, nan), (9, 0.5), (10, -1.0), (11, nan), (12, 0.99), (12, nan),
                 (13, 0.0), (14, 2.0), (15, nan), (16, -1.0), (16, nan), (17, 0)):
        bad = list(good)
        bad[i] = v
        if (i, v) == (5, 65536):
            bad[6] = 65536
        if (i, v) == (14, 2.0):
            bad[15] = 1.0
        assert lib.rtgs_white_balance_fit(*bad) == E, (i, v)
    ok = [p(d[0]), 60, 80, p(state), p(out[0]), p(out[1]), st]
    for i, v in ((0, None), (3, None), (4, None), (5, None), (1, 0), (2, -3), (4, p(d[0])), (5, p(d[0]))):
        bad = list(ok)
        bad[i] = v
        assert lib.rtgs_white_balance_apply(*bad) == E, (i, v)
    torch.cuda.synchronize()
    assert torch.equal(state, before)


def test_apply_writes_both_layouts_into_new_storage():
    from rtg_slam_amd import map_exposure as me
    rng = np.random.default_rng(7)
    c = rng.random((3, 37, 53)).astype(F32)
    c[0, 0, :4] = (0.0, 1.0, 0.5, 0.999)
    c[1, 5, 6], c[2, 7, 8] = np.nan, np.inf
    ab = ((9.0, 9.0), (1.3, -0.1), (0.8, 0.3), (1.0, 0.0))
    m = me.MapExposure(SimpleNamespace(map_exposure_channels="rgb"), DEV)
    assert m.state.numel() == me.WB_STATE
    for k, (a, b) in enumerate(ab):
        m.state[8 * k], m.state[8 * k + 1] = a, b
    t = dev(c)
    chw, hwc = m.apply(t)
    want_chw, want_hwc = wbr.apply(c, ab)
    assert np.array_equal(bits32(chw.cpu().numpy()), bits32(want_chw))
    assert np.array_equal(bits32(hwc.cpu().numpy()), bits32(want_hwc))
    assert chw.shape == (3, 37, 53) and hwc.shape == (37, 53, 3) and chw.is_contiguous() and hwc.is_contiguous()
    assert np.array_equal(t.cpu().numpy(), c, equal_nan=True)                   # the input is not written
    assert len({t.data_ptr(), chw.data_ptr(), hwc.data_ptr()}) == 3
    assert float(chw[1, 5, 6]) == 0.0 and float(chw[2, 7, 8]) == 1.0            # a NaN becomes 0
    assert (want_chw == 0).any() and (want_chw == 1).any()


def test_history_and_report_carry_the_channels():
    from rtg_slam_amd import map_exposure as me
    m = me.MapExposure(SimpleNamespace(map_exposure_channels="rgb"), DEV)
    m.skip()
    good = wbr.scene(60, 80, (1.25, 0.8, 1.0), (-0.06, 0.08, 0.0))
    for sc in (good, wbr.constant_channel_scene(channel=2), wbr.scene(clean=np.full((3, 60, 80), 0.5, F32))):
        m.fit(dev(sc["src_color"]), dev(sc["src_depth"]), {"render": dev(sc["dst_color"]), "depth": dev(sc["dst_depth"]),
                                                           "T_map": dev(sc["T_map"])})
    h = m.history()
    ab, _, _, steps = wbr.fit(**good)
    assert h[0] == (1.0, 0.0, 0, 0, 0, 1.0, 0.0, 0, 1.0, 0.0, 0, 1.0, 0.0, 0)
    assert h[1] == (ab[0][0], ab[0][1], 0, int(steps[-1]["S"][28]), int(steps[-1]["S"][6]), ab[1][0], ab[1][1], 0, ab[2][0], ab[2][1], 0,
                    ab[3][0], ab[3][1], 0)
    assert h[2][2] == 0 and h[2][13] == wbr.FLAT and h[2][11:13] == h[2][0:2]
    assert h[3][2] == wbr.FLAT and h[3][:2] == h[2][:2] and h[3][5:7] == h[2][5:7]
    rep = m.report()
    assert rep["channels"] == "rgb" and rep["options"]["channels"] == "rgb"
    assert rep["frames_fitted"] == 3 and rep["frames_fell_back"] == 1 and rep["fell_back"] == {"3": "no variance of intensity"}
    assert rep["followed_grey_b"] == 1 and rep["followed_grey_r"] == 0
    assert rep["alpha_r_min"] <= rep["alpha_r_mean"] <= rep["alpha_r_max"] and rep["beta_g_min"] <= rep["beta_g_max"]
    grey = grey_gpu.stage()
    assert "channels" not in grey.report() and "channels" not in grey.options() and grey.state.numel() == me.STATE


# ---- the mapper ----

FRAMES = grey_gpu.FRAMES
# What a camera with auto exposure AND auto white balance does: the grey test's exposure per frame (GAINS: 1.2 / -0.03 and 0.85 /
# 0.02 in turn) times a tint that warms the bright frames and cools the dark ones.  The common part is what a grey fit can remove
# (so grey < off has a reason), the tint what only a fit per channel can (rgb < grey).  A tint that leaves the luma where it was -
# (1.2, 0.9, 1.05) against (0.85, 1.1, 0.95), grey gain 1.007 and 0.008 - gives the grey fit nothing to remove: measured on an
# MI355X 0.00947 with the option off, 0.00994 with grey, 0.00567 with rgb; it is not asserted here.
WARM, COOL = (1.08, 1.0, 0.92), (0.93, 1.0, 1.08)
TINTS = [((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))] + [(tuple(g * t for t in (WARM if k % 2 else COOL)), (o, o, o))
                                                for k, (g, o) in enumerate(grey_gpu.GAINS) if k > 0]


def _gains():
    """TINTS as (gain, offset) tensors [3,1,1] that the grey harness's stream multiplies and adds channel by channel."""
    t = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV).reshape(3, 1, 1)
    return [(t(g), t(o)) for g, o in TINTS]


def test_mapper_keeps_the_map_in_one_white_balance():
    """Twelve box-room frames at GT poses under alternating per-channel gains (the harness of tests/test_map_exposure_gpu.py).
    Mean absolute colour error of the final map, rendered at the twelve poses, against the clean colour, printed for the three
    arms: rgb < grey < off.  On an MI355X, three runs: off 0.01182-0.01203, grey 0.01139-0.01142, rgb 0.00616-0.00618 (the map
    step adds gradients in arrival order, so the figures move in the fourth digit from run to run)."""
    gains = _gains()
    _, _, rep_off, _, _, e_off = grey_gpu._run(grey_gpu._args(), gains)
    _, _, rep_grey, _, _, e_grey = grey_gpu._run(grey_gpu._args(map_exposure=True), gains)
    mapper, _, rep, given, seen, e_rgb = grey_gpu._run(grey_gpu._args(map_exposure=True, map_exposure_channels="rgb"), gains)
    print(f"map colour error against the clean colour: option off {e_off:.5f}, grey {e_grey:.5f}, rgb {e_rgb:.5f}")
    hist = mapper.map_exposure.history()
    for c, name in enumerate("rgb"):
        print(f"alpha_{name} per frame:", [round(h[5 + 3 * c], 4) for h in hist], "for 1 / gain", [round(1 / g[c], 4) for g, _ in TINTS])
    assert e_rgb < e_grey
    assert e_grey < e_off
    assert "map_exposure" not in rep_off and "channels" not in rep_grey["map_exposure"] and rep["map_exposure"]["channels"] == "rgb"
    assert len(hist) == FRAMES and rep["map_exposure"]["frames_fitted"] == FRAMES - 1 and rep["map_exposure"]["frames_fell_back"] == 0
    for k in range(1, FRAMES):
        assert hist[k][2] == 0 and len(hist[k]) == 14, (k, hist[k])
        for c in range(3):
            g = TINTS[k][0][c]
            assert abs(hist[k][5 + 3 * c] - 1 / g) < abs(1 - 1 / g), (k, c, hist[k])
        assert seen[k]["color_raw_chw"] is given[k] and seen[k]["color_chw"].data_ptr() != given[k].data_ptr()
        assert torch.equal(seen[k]["color_map"], seen[k]["color_chw"].permute(1, 2, 0))


def test_absent_key_is_the_grey_path_call_for_call(monkeypatch):
    """With map_exposure_channels absent the grey entry points are called as tests/test_map_exposure_gpu.py::test_off_means_off
    counts them - 5 frames x 4 iterations, 5 applies over six frames - and no rtgs_white_balance_* entry is; with rgb it is the
    other way round."""
    from rtg_slam_amd import _lib
    lib = _lib.load()
    calls = {n: 0 for n in grey_gpu.NEW_ENTRIES + WB_ENTRIES}

    def counted(name, fn):
        def wrapper(*a):
            calls[name] += 1
            return fn(*a)
        return wrapper

    for name in calls:
        monkeypatch.setattr(lib, name, counted(name, getattr(lib, name)))
    args = grey_gpu._args(gaussian_update_iter=0, map_exposure=True)
    assert not hasattr(args, "map_exposure_channels")
    grey_gpu._run(args, _gains(), n=6)
    assert calls["rtgs_map_exposure_fit"] == 5 * 4 and calls["rtgs_map_exposure_apply"] == 5
    assert all(calls[n] == 0 for n in WB_ENTRIES)
    before = dict(calls)
    grey_gpu._run(grey_gpu._args(gaussian_update_iter=0, map_exposure=True, map_exposure_channels="rgb"), _gains(), n=6)
    assert calls["rtgs_white_balance_fit"] == 5 * 4 and calls["rtgs_white_balance_apply"] == 5
    assert all(calls[n] == before[n] for n in grey_gpu.NEW_ENTRIES)
