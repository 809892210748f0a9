"""The definition of the mapper's exposure stage, tests/map_exposure_reference.py, on its own: what it recovers, why its first
iteration is plain Huber, when it falls back, what each gate removes; and the plumbing (config keys, `slam --map-exposure`, the
pipeline's refusal).  No GPU.  tests/test_map_exposure_gpu.py holds the kernels to the same cases bit for bit."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import map_exposure_reference as mer

F32 = np.float32
# Recovery: the frame is an exact affine image of the render up to float32 rounding of gain c + offset (relative 6e-8 per step),
# so the fit ends at the truth up to that; measured on the definition: at most 6.9e-8 over the five cases.  15 x margin.
RECOVERY_TOL = 1e-6
# Robustness (frozen): the image of mer.textured(), 20 % of the pixels a random colour, gain 0.8 and offset -0.08, seeds 0..4.
# Measured on the definition: the schedule ends within 0.0136-0.0172 of the truth, four plain Huber iterations 0.147-0.174 away.
ROBUST_CASE = (0.8, -0.08)
SCHEDULE_BOUND, HUBER_BOUND = 0.03, 0.1
# Cut from the start (frozen): the brighter image mer.textured(lo=0.55, amp=0.3), gain 1.25, offset 0.08, start (1, 0): the
# residual there is 0.25 c + 0.08 >= 0.14 against a cut of 0.15, so iteration 0 keeps almost no inlier and fits the outliers.
# Measured: 0.161-0.448 from the truth after the schedule's four iterations, where the schedule itself is within 0.033-0.042.
CUT_START_CASE = (1.25, 0.08)
CUT_START_BOUND, CUT_SCHEDULE_BOUND = 0.1, 0.05


def truth(g, o):
    return 1.0 / g, -o / g


def off(state, g, o):
    a, b = truth(g, o)
    return max(abs(state[0] - a), abs(state[1] - b))


def huber_only(a, huber, cut, iteration):
    return mer.weights(a, huber, cut, 0)


def cut_always(a, huber, cut, iteration):
    return mer.weights(a, huber, cut, 1)


@pytest.mark.parametrize("gain,offset", mer.RECOVERY_CASES)
def test_exact_recovery(gain, offset):
    s = mer.scene(60, 80, gain, offset)
    state, code, steps = mer.fit(**s)
    print(f"gain {gain} offset {offset}: alpha {state[0]!r} beta {state[1]!r}, off by {off(state, gain, offset):.3g}")
    assert code == mer.OK and len(steps) == 4
    assert off(state, gain, offset) <= RECOVERY_TOL
    assert steps[-1][0][6] >= 0.8 * 4800                                      # the clamp's gate removes some at a gain above 1


@pytest.mark.parametrize("seed", mer.ROBUST_SEEDS)
def test_schedule_survives_outliers_where_plain_huber_does_not(seed):
    g, o = ROBUST_CASE
    s = mer.scene(60, 80, g, o, outliers=0.2, seed=seed)
    sched, code, _ = mer.fit(**s)
    plain, code_p, _ = mer.fit(**s, weight_fn=huber_only)
    print(f"seed {seed}: schedule off by {off(sched, g, o):.4f}, four Huber iterations off by {off(plain, g, o):.4f}")
    assert code == mer.OK and code_p == mer.OK
    assert off(sched, g, o) <= SCHEDULE_BOUND
    assert off(plain, g, o) > HUBER_BOUND


@pytest.mark.parametrize("seed", mer.ROBUST_SEEDS)
def test_cut_weight_from_the_start_does_not_converge(seed):
    """The reason for the schedule.  With the definition's weight (Huber with a cut, not Tukey) the cut start does not run away:
    it fits the outliers first and crawls back - it is where the schedule ends only after about eight iterations."""
    g, o = CUT_START_CASE
    s = mer.scene(60, 80, g, o, outliers=0.2, seed=seed, clean=mer.textured(60, 80, lo=0.55, amp=0.3))
    cut0, _, _ = mer.fit(**s, weight_fn=cut_always)
    sched, code, _ = mer.fit(**s)
    print(f"seed {seed}: cut from iteration 0 off by {off(cut0, g, o):.4f}, the schedule by {off(sched, g, o):.4f}")
    assert off(cut0, g, o) > CUT_START_BOUND
    assert code == mer.OK and off(sched, g, o) <= CUT_SCHEDULE_BOUND


START = (0.9, 0.02)


def fallback_scenes():
    few = mer.scene()
    few["frame_depth"][:, 1:] = 0                                             # 60 valid pixels, min_valid is 64
    return {"constant frame": (mer.scene(clean=np.full((3, 60, 80), 0.5, F32)), mer.FLAT),
            "too few valid pixels": (few, mer.TOO_FEW),
            "gain 5": (mer.scene(gain=5.0, clean=mer.textured(lo=0.1, amp=0.07)), mer.RANGE)}


@pytest.mark.parametrize("name", ["constant frame", "too few valid pixels", "gain 5"])
def test_fallbacks_return_the_frame_start_and_their_code(name):
    s, want = fallback_scenes()[name]
    state, code, steps = mer.fit(**s, state=START)
    assert code == want and state == START
    assert [st[3] for st in steps] == [want] * 4
    assert all(np.array_equal(st[0], steps[0][0]) for st in steps)            # the later iterations are no-ops


GATES = {"frame depth hole": lambda s: s["frame_depth"].__setitem__((10, 20), 0.0),
         "render depth hole": lambda s: s["render_depth"].__setitem__((10, 20), 0.0),
         "depth disagreement": lambda s: s["render_depth"].__setitem__((10, 20), 2.06),
         "transparent": lambda s: s["T_map"].__setitem__((10, 20), 0.2),
         "clamped high": lambda s: s["frame_color"].__setitem__((1, 10, 20), 1.0),
         "clamped low": lambda s: s["frame_color"].__setitem__((2, 10, 20), 0.0),
         "render not finite": lambda s: s["render_color"].__setitem__((0, 10, 20), np.inf)}


@pytest.mark.parametrize("gate", sorted(GATES))
def test_each_gate_alone_removes_its_pixel(gate):
    s = mer.scene()
    assert mer.valid_mask(**s).sum() == 4800
    GATES[gate](s)
    v = mer.valid_mask(**s)
    assert v.sum() == 4799 and not v[10, 20]
    assert mer.fit(**s, iters=1)[2][0][0][6] == 4799.0
    # just inside the gates the pixel stays
    s = mer.scene()
    s["render_depth"][10, 20] = 2.04
    s["T_map"][10, 20] = 0.1
    assert mer.valid_mask(**s).sum() == 4800


def test_gated_scene_exercises_every_gate():
    s = mer.gated_scene()
    v = mer.valid_mask(**s)
    assert 0.6 * 4800 < v.sum() < 0.9 * 4800
    assert (s["frame_depth"] == 0).any() and (s["render_depth"] == 0).any() and (s["T_map"] > 0.1).any()
    assert np.isnan(s["render_color"]).any() and (s["frame_color"] == 1).any() and (s["frame_color"] == 0).any()
    state, code, _ = mer.fit(**s)
    assert code == mer.OK and off(state, 1.2, -0.03) <= RECOVERY_TOL


def test_apply_clamps_both_ends_and_leaves_the_input():
    c = np.linspace(0, 1, 3 * 4 * 5, dtype=F32).reshape(3, 4, 5)
    keep = c.copy()
    chw, hwc = mer.apply(c, 1.5, -0.2)
    assert chw.min() == 0 and chw.max() == 1 and np.array_equal(c, keep)
    assert hwc.shape == (4, 5, 3) and np.array_equal(hwc.transpose(2, 0, 1), chw)
    mid = (chw > 0) & (chw < 1)
    assert mid.any() and np.array_equal(chw[mid], (F32(1.5) * c + F32(-0.2))[mid])


# ---- plumbing ----

def test_config_keys_parse(tmp_path):
    from rtg_slam_amd import config, mapping as mp
    for preset in (mp.replica_args, mp.tum_args, mp.scannetpp_args):
        assert not any(k.startswith("map_exposure") for k in vars(preset()))   # absent from the presets
    p = tmp_path / "c.yaml"
    p.write_text('parent: "None"\ntype: Replica\nmap_exposure: true\nmap_exposure_iters: 5\nmap_exposure_huber: 0.04\n'
                 "map_exposure_cut: 2.5\nmap_exposure_depth_gate: 0.03\nmap_exposure_t_gate: 0.2\n")
    args = config.load_config(str(p))
    assert args.map_exposure is True and args.map_exposure_iters == 5 and args.map_exposure_huber == 0.04
    assert args.map_exposure_cut == 2.5 and args.map_exposure_depth_gate == 0.03 and args.map_exposure_t_gate == 0.2


def test_defaults_are_the_stated_ones():
    from rtg_slam_amd import map_exposure as me, rgbd_align
    d = me.DEFAULTS
    assert d["map_exposure_iters"] == 4 and d["map_exposure_huber"] == rgbd_align.DEFAULT_HUBER == 0.05
    assert d["map_exposure_cut"] == 3 and d["map_exposure_depth_gate"] == 0.05 and d["map_exposure_t_gate"] == 0.1
    assert d["map_exposure_lo"] == 4 / 255 and d["map_exposure_hi"] == 251 / 255 and d["map_exposure_var_min"] == 1e-4
    assert me.min_valid_default(60, 80) == 64 and me.min_valid_default(680, 1200) == 8160
    for k, v in mer.DEFAULTS.items():
        assert d["map_exposure_" + k] == v
    assert me.min_valid_default(240, 320) == mer.min_valid_default(240, 320)


def test_slam_flag_reaches_the_args_and_the_dumped_config(tmp_path):
    import yaml
    from rtg_slam_amd import __main__ as cli
    on = cli.build_parser().parse_args(["slam", "--config", "x.yaml", "--map-exposure"])
    off_ = cli.build_parser().parse_args(["slam", "--config", "x.yaml"])
    args = SimpleNamespace(save_path="x")
    cli._apply_map_exposure(args, off_)
    assert not hasattr(args, "map_exposure")
    cli._apply_map_exposure(args, on)
    assert args.map_exposure is True
    cli._dump_config(args, str(tmp_path / "config.yaml"))
    assert yaml.safe_load(open(tmp_path / "config.yaml"))["map_exposure"] is True


def test_pipeline_refuses_the_option():
    from rtg_slam_amd import map_exposure as me
    me.refuse_pipeline(SimpleNamespace())
    me.refuse_pipeline(SimpleNamespace(map_exposure=False))
    with pytest.raises(ValueError, match="map_exposure is not built"):
        me.refuse_pipeline(SimpleNamespace(map_exposure=True))


def test_header_declares_the_entry_points_without_a_new_struct():
    from rtg_slam_amd import _lib
    names = [n for n in _lib.EXPORTED_SYMBOLS if n.startswith("rtgs_map_exposure_")]
    assert sorted(names) == ["rtgs_map_exposure_apply", "rtgs_map_exposure_fit", "rtgs_map_exposure_scratch_bytes"]
    assert len(_lib.STRUCTS) == 7
    assert os.path.exists(os.path.join(os.path.dirname(_lib.INCLUDE_DIR), "rtg_slam_amd", "csrc", "map_exposure.hip"))
