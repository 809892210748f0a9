"""The definition of the white balance fit, tests/white_balance_reference.py, on its own: what it recovers per channel and what a
grey fit cannot, that it survives outliers, the frame rule; and the plumbing (`map_exposure_channels`, `slam
--map-exposure-channels`, the header).  No GPU.  tests/test_white_balance_gpu.py holds the kernels to the same cases bit for bit."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import map_exposure_reference as mer
from tests import test_map_exposure_cpu as grey_cpu
from tests import white_balance_reference as wbr

F32 = np.float32
CASES = range(len(mer.RECOVERY_CASES))
# Robustness: the channels carry (0.8, -0.08) - the grey test's ROBUST_CASE - (1.25, -0.06) and (0.8, 0.08), 20 % of the pixels a
# random colour, seeds 0..4, the grey test's bounds.  Measured on the definition: the schedule ends within 0.0055-0.0153 of the
# truth on every channel; four plain Huber iterations are 0.250-0.273 away on the ROBUST_CASE channel (0.051-0.146 on the others).
ROBUST_CHANNELS = (grey_cpu.ROBUST_CASE, (1.25, -0.06), (0.8, 0.08))
START = ((0.9, 0.02), (1.1, -0.01), (0.95, 0.0), (1.0, 0.03))


def off(ab, g, o):
    return grey_cpu.off(ab, g, o)


_bound = []


def recovery_bound():
    """Twice the grey definition's own worst recovery error over RECOVERY_CASES on mer.scene(60, 80): a channel sees a third of the
    luma's averaging.  Computed once."""
    if not _bound:
        worst = max(off(mer.fit(**mer.scene(60, 80, g, o))[0], g, o) for g, o in mer.RECOVERY_CASES)
        _bound.append(2.0 * worst)
    return _bound[0]


def tinted_scene(k):
    cs = wbr.channel_cases(k)
    return cs, wbr.scene(60, 80, [c[0] for c in cs], [c[1] for c in cs])


@pytest.mark.parametrize("k", CASES)
def test_every_channel_recovers_its_own_gain_and_offset(k):
    """Channel j of case k carries RECOVERY_CASES[(k + j) % 5]: three different pairs.  Measured: the grey definition's worst error
    over the five cases is 6.83e-8, so the bound is 1.37e-7; the worst channel error over the five cases is 6.66e-8."""
    cs, s = tinted_scene(k)
    ab, codes, frame, steps = wbr.fit(**s)
    errs = [off(ab[j + 1], *cs[j]) for j in range(3)]
    print(f"case {k}: channel errors {errs}, bound {recovery_bound():.3g}")
    assert frame == wbr.OK and codes == [wbr.OK] * 4 and len(steps) == 4
    assert len(set(cs)) == 3
    assert max(errs) <= recovery_bound()
    assert steps[-1]["S"][wbr.VALID] >= 0.6 * 4800                            # the clamp's gate removes some at a gain above 1


@pytest.mark.parametrize("k", CASES)
def test_grey_fit_leaves_a_tint(k):
    """The reason for the feature: one (alpha, beta) on the grey values cannot be right for three channels at different gains.
    Measured: the worst channel is 0.23-0.37 from its truth, the bound is 1.37e-7."""
    cs, s = tinted_scene(k)
    state, code, _ = mer.fit(**wbr.as_grey(s))
    errs = [off(state, *cs[j]) for j in range(3)]
    print(f"case {k}: the grey fit's (alpha, beta) is {errs} from the channels' truths")
    assert code == mer.OK
    assert max(errs) > recovery_bound()
    ab, _, _, _ = wbr.fit(**s)                                                # and regression 0 IS that grey fit
    assert ab[0] == state


@pytest.mark.parametrize("seed", mer.ROBUST_SEEDS)
def test_schedule_survives_outliers_on_every_channel(seed):
    cs = ROBUST_CHANNELS
    s = wbr.scene(60, 80, [c[0] for c in cs], [c[1] for c in cs], outliers=0.2, seed=seed)
    sched, codes, frame, _ = wbr.fit(**s)
    plain, _, frame_p, _ = wbr.fit(**s, weight_fn=grey_cpu.huber_only)
    e_s = [off(sched[j + 1], *cs[j]) for j in range(3)]
    e_p = [off(plain[j + 1], *cs[j]) for j in range(3)]
    print(f"seed {seed}: schedule off by {e_s}, four Huber iterations off by {e_p}")
    assert frame == wbr.OK and frame_p == wbr.OK and codes == [wbr.OK] * 4
    assert max(e_s) <= grey_cpu.SCHEDULE_BOUND
    assert e_p[0] > grey_cpu.HUBER_BOUND
    assert all(p > q for p, q in zip(e_p, e_s))


def test_constant_channel_is_refused_and_follows_the_grey():
    s = wbr.constant_channel_scene(channel=2)
    ab, codes, frame, steps = wbr.fit(**s, state=START)
    assert frame == wbr.OK and codes == [wbr.OK, wbr.OK, wbr.OK, wbr.FLAT]
    for st in steps:                                                          # from iteration 0 on, and it keeps its code
        assert st["codes"][3] == wbr.FLAT and st["ab"][3] == st["ab"][0] and st["frame"] == wbr.OK
    assert steps[-1]["iters"] == [4, 4, 4, 0]
    assert ab[3] == ab[0] and ab[3] != START[3]
    assert off(ab[1], 1.25, -0.06) <= recovery_bound() and off(ab[2], 0.8, 0.08) <= recovery_bound()
    g, _, _ = mer.fit(**wbr.as_grey(s), state=START[0])                       # the grey it follows is the grey fit's
    assert ab[0] == g


def test_too_few_valid_pixels_restores_all_four():
    few = wbr.scene(gains=(1.25, 0.8, 1.0), offsets=(-0.06, 0.08, 0.0))
    few["src_depth"][:, 1:] = 0                                               # 60 valid pixels, min_valid is 64
    ab, codes, frame, steps = wbr.fit(**few, state=START)
    assert frame == wbr.TOO_FEW and codes == [wbr.TOO_FEW] * 4
    assert [tuple(map(float, p)) for p in ab] == list(START)
    assert all(st["frame"] == wbr.TOO_FEW and st["iters"] == [0] * 4 for st in steps)
    assert all(np.array_equal(st["S"], steps[0]["S"]) for st in steps)        # the later iterations are no-ops
    assert steps[0]["S"][wbr.VALID] == 60.0


def test_refused_grey_ends_the_frame_for_every_channel():
    s = wbr.scene(clean=np.full((3, 60, 80), 0.5, F32))
    ab, codes, frame, steps = wbr.fit(**s, state=START)
    assert frame == wbr.FLAT and codes == [wbr.FLAT] * 4
    assert [tuple(map(float, p)) for p in ab] == list(START)
    s = wbr.scene(gains=(5.0, 5.0, 1.0), clean=mer.textured(lo=0.1, amp=0.07))   # the grey out of range, blue fine on its own
    ab, codes, frame, _ = wbr.fit(**s, state=START)
    assert frame == wbr.RANGE and codes == [wbr.RANGE, wbr.RANGE, wbr.RANGE, wbr.OK]
    assert [tuple(map(float, p)) for p in ab] == list(START)


def test_dst_bounds_gate_the_target_and_infinite_ones_reduce_to_finite():
    s = wbr.scene()
    assert wbr.valid_mask(**s).sum() == 4800
    s["dst_color"][1, 10, 20] = 1.0
    assert wbr.valid_mask(**s).sum() == 4800
    v = wbr.valid_mask(**s, dst_lo=4 / 255, dst_hi=251 / 255)
    assert v.sum() == 4799 and not v[10, 20]
    s["dst_color"][1, 10, 20] = np.inf
    assert wbr.valid_mask(**s).sum() == 4799
    s["src_color"][0, 3, 4] = np.nan
    assert wbr.valid_mask(**s, src_lo=-np.inf, src_hi=np.inf).sum() == 4798
    g = wbr.gated_scene()
    assert np.array_equal(wbr.valid_mask(**g), mer.valid_mask(**wbr.as_grey(g)))
    assert wbr.valid_mask(**g, dst_lo=4 / 255, dst_hi=251 / 255).sum() < wbr.valid_mask(**g).sum()


def test_apply_is_per_channel_and_clamps():
    c = np.linspace(0, 1, 3 * 4 * 5, dtype=F32).reshape(3, 4, 5)
    c[1, 0, 0] = np.nan
    keep = c.copy()
    ab = ((9.0, 9.0), (1.5, -0.2), (0.5, 0.1), (1.0, 0.6))
    chw, hwc = wbr.apply(c, ab)
    assert np.array_equal(c, keep, equal_nan=True) and chw[1, 0, 0] == 0
    assert hwc.shape == (4, 5, 3) and np.array_equal(hwc.transpose(2, 0, 1), chw)
    for k in range(3):
        want, _ = mer.apply(c, *ab[k + 1])
        assert np.array_equal(chw[k], want[k])
    assert chw.min() == 0 and chw.max() == 1


# ---- plumbing ----

def test_config_key_parses_and_is_absent_from_every_preset(tmp_path):
    from rtg_slam_amd import config, map_exposure as me, mapping as mp
    for preset in (mp.replica_args, mp.tum_args, mp.scannetpp_args):
        assert not hasattr(preset(), "map_exposure_channels")
    p = tmp_path / "c.yaml"
    p.write_text('parent: "None"\ntype: Replica\nmap_exposure: true\nmap_exposure_channels: rgb\n')
    args = config.load_config(str(p))
    assert args.map_exposure_channels == "rgb" and me.channels_of(args) == "rgb"
    assert me.channels_of(SimpleNamespace()) == "grey" and me.channels_of(SimpleNamespace(map_exposure_channels="grey")) == "grey"
    with pytest.raises(ValueError, match="map_exposure_channels"):
        me.channels_of(SimpleNamespace(map_exposure_channels="hsv"))


def test_grey_constructs_nothing_new(monkeypatch):
    """Without a GPU the object cannot be built, so the constructor runs on a stand-in for torch's allocation: absent and `grey`
    allocate the RTGS_MAP_EXPOSURE_STATE doubles and nothing else, `rgb` the RTGS_WHITE_BALANCE_STATE doubles."""
    import torch
    from rtg_slam_amd import _lib, map_exposure as me
    made = []
    real = torch.zeros

    def zeros(*shape, **kw):
        kw.pop("device", None)
        made.append(int(np.prod(shape)))
        return real(*shape, **kw)

    monkeypatch.setattr(me.torch, "zeros", zeros)
    monkeypatch.setattr(_lib, "load", lambda: None)
    for over, want in (({}, [me.STATE]), ({"map_exposure_channels": "grey"}, [me.STATE]),
                       ({"map_exposure_channels": "rgb"}, [me.WB_STATE])):
        made.clear()
        m = me.MapExposure(SimpleNamespace(**over), "cuda:0")
        assert made == want and m.channels == over.get("map_exposure_channels", "grey")
        assert "channels" not in m.options() or m.channels == "rgb"
    assert me.STATE == 16 and me.WB_STATE == 72


def test_slam_flag_is_written_only_when_given_and_refused_without_map_exposure(tmp_path, capsys):
    import yaml
    from rtg_slam_amd import __main__ as cli
    parse = cli.build_parser().parse_args
    absent = parse(["slam", "--config", "x.yaml", "--map-exposure"])
    rgb = parse(["slam", "--config", "x.yaml", "--map-exposure", "--map-exposure-channels", "rgb"])
    args = SimpleNamespace(save_path="x", map_exposure=True)
    assert cli._apply_map_exposure_channels(args, absent) is None and not hasattr(args, "map_exposure_channels")
    assert cli._apply_map_exposure_channels(args, rgb) is None and args.map_exposure_channels == "rgb"
    cli._dump_config(args, str(tmp_path / "config.yaml"))
    assert yaml.safe_load(open(tmp_path / "config.yaml"))["map_exposure_channels"] == "rgb"
    with pytest.raises(SystemExit):
        parse(["slam", "--config", "x.yaml", "--map-exposure", "--map-exposure-channels", "hsv"])
    # the command itself: exit code 2 before anything is created or any device is touched
    cfg = tmp_path / "c.yaml"
    out = tmp_path / "out"
    cfg.write_text(f'parent: "None"\ntype: Replica\nsave_path: {out}\n')
    assert cli.main(["slam", "--config", str(cfg), "--map-exposure-channels", "rgb"]) == 2
    assert not out.exists()


def test_header_declares_exactly_the_three_entry_points():
    from rtg_slam_amd import _lib
    names = sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith("rtgs_white_balance_"))
    assert names == ["rtgs_white_balance_apply", "rtgs_white_balance_fit", "rtgs_white_balance_scratch_bytes"]
    grey = sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith("rtgs_map_exposure_"))
    assert grey == ["rtgs_map_exposure_apply", "rtgs_map_exposure_fit", "rtgs_map_exposure_scratch_bytes"]
    assert len(_lib.STRUCTS) == 7
    c = _lib.CONSTANTS
    assert c["RTGS_WHITE_BALANCE_REGRESSIONS"] * c["RTGS_WHITE_BALANCE_REG"] == c["RTGS_WHITE_BALANCE_FRAME_AT"] == 32
    assert c["RTGS_WHITE_BALANCE_SUMS_AT"] + c["RTGS_WHITE_BALANCE_SUMS"] == c["RTGS_WHITE_BALANCE_STATE"] == 72
    assert c["RTGS_WHITE_BALANCE_VALID"] == wbr.VALID == 28 and c["RTGS_WHITE_BALANCE_SUMS"] == wbr.OUT
    assert c["RTGS_MAP_EXPOSURE_STATE"] == 16
    assert os.path.exists(os.path.join(os.path.dirname(_lib.INCLUDE_DIR), "rtg_slam_amd", "csrc", "white_balance.hip"))
