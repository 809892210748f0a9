"""tests/rgbd_exposure_reference.py, the numpy definition of the exposure-compensated RGB-D refinement, against
tests/rgbd_align_reference.py and against what it is for: a flat textured wall whose source frame was taken at another exposure."""
import numpy as np
import pytest

from tests import rgbd_align_reference as rar
from tests import rgbd_exposure_reference as rer

NAMES = ("v_src", "n_src", "i_src", "v_tgt", "n_tgt", "i_tgt")
DIST, COS = 0.1, float(np.cos(np.deg2rad(20.0)))
SIZES = [(60, 80), (30, 40)]
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def run6(s, iters=12):
    return rar.refine(np.eye(4), *[[s[k]] for k in NAMES], s["K"], [1.0], iters=[iters], distance_threshold=DIST, cos_threshold=COS)


def run8(s, iters=12):
    return rer.refine(np.eye(4), *[[s[k]] for k in NAMES], s["K"], [1.0], iters=[iters], distance_threshold=DIST, cos_threshold=COS)


def offset_mm(T, truth):
    return 1e3 * float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


@pytest.mark.parametrize("H,W", SIZES)
def test_unit_exposure_gives_the_six_unknown_sums(H, W):
    s = rar.wall_pair(H, W)
    s["n_src"][H // 2:H // 2 + 3] = 0                                         # the geometric gate fails where the photometric passes
    for pose in (np.eye(4), rar.se3_exp(rar.WALL_XI)):
        want = rar.accumulate(*[s[k] for k in NAMES], s["K"], pose, DIST, COS, 0.25, 0.05)
        got = rer.accumulate(*[s[k] for k in NAMES], s["K"], pose, DIST, COS, 0.25, 0.05, 1.0, 0.0)
        assert got.shape == (48,) and 0 < want[28] < want[30]
        assert np.array_equal(bits(rer.pose_block(got)), bits(want))
        assert got[6] != 0 and 0 < got[35] <= want[30] * 0.0625               # the new entries are filled: H[7,7] = sum w lambda^2


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("gain,offset", rer.EXPOSURE_CASES)
def test_eight_unknowns_recover_the_wall_at_another_exposure(H, W, gain, offset):
    s = rer.exposed_wall_pair(H, W, gain, offset)
    truth = s["truth"]
    start = offset_mm(np.eye(4), truth)
    assert abs(start - 26.93) < 0.01
    T6, _ = run6(s)
    T8, rep = run8(s)
    e6, e8 = offset_mm(T6, truth), offset_mm(T8, truth)
    alpha, beta = rep["exposure"]
    print(f"{W}x{H} gain {gain} offset {offset}: six unknowns {e6:.3f} mm, eight {e8:.3f} mm of {start:.2f}; alpha {alpha:.4f} "
          f"beta {beta:.4f} for {1 / gain:.4f} {-offset / gain:.4f}")
    if (gain, offset) == (1.25, -0.06):
        assert e6 >= 0.25 * start                                             # precondition: the exposure does break the six-unknown loop
        assert e8 <= 0.1 * e6
    assert e8 <= 0.05 * start
    assert rep["rank"] and all(r == 8 for r in rep["rank"]) and rep["reason"] == "done"
    assert abs(alpha - 1 / gain) <= 0.03 and abs(beta + offset / gain) <= 0.03
    assert rep["exposure_steps"][-1] == rep["exposure"] and len(rep["exposure_steps"]) == sum(rep["iterations"])


def test_textureless_wall_leaves_the_exposure_alone():
    s = rer.exposed_wall_pair(60, 80, textured=False)
    T, rep = run8(s, iters=3)
    assert rep["iterations"] == [3] and rep["rank"] == [4, 4, 4]
    assert rep["exposure"] == (1.0, 0.0) and rep["reason"] == "done"
    assert np.isfinite(T).all()


def test_exposure_out_of_range_stops_the_loop():
    s = rer.exposed_wall_pair(60, 80, 8.0, 0.0)                               # the gain that undoes it, 0.125, is below 0.25
    T, rep = run8(s)
    assert rep["reason"] == "exposure out of range"
    assert rep["exposure"] == (1.0, 0.0)
    assert len(rep["rank"]) == sum(rep["iterations"]) + 1
    # the pose is the one before the refused update
    again = rer.refine(np.eye(4), *[[s[k]] for k in NAMES], s["K"], [1.0], iters=[sum(rep["iterations"])], distance_threshold=DIST,
                       cos_threshold=COS)[0] if sum(rep["iterations"]) else np.eye(4)
    assert np.array_equal(bits(T), bits(again))
    assert not rer.in_range(0.2, 0.0) and not rer.in_range(1.0, -0.51) and not rer.in_range(float("nan"), 0.0)
    assert rer.in_range(0.25, 0.5) and rer.in_range(4.0, -0.5)


def test_composite_target():
    rng = np.random.default_rng(3)
    render, frame = rng.random((3, 4, 6)).astype(F32), rng.random((3, 4, 6)).astype(F32)
    rendered = (1 + rng.random((4, 6))).astype(F32)
    rendered[1:3, 2:5] = 0                                                    # a hole of the model
    filled = rendered.copy()
    filled[1:3, 2:5] = (2 + rng.random((2, 3))).astype(F32)                   # filled from the frame
    block = np.zeros((4, 6), bool)
    block[1:3, 2:5] = True
    unit = rer.composite(render, frame, rendered, filled, 1.0, 0.0)
    assert unit.dtype == F32
    assert np.array_equal(unit[block].view(np.int32), rar.grey(frame)[block].view(np.int32))
    assert np.array_equal(unit[~block].view(np.int32), rar.grey(render)[~block].view(np.int32))
    got = rer.composite(render, frame, rendered, filled, 0.8, 0.05)
    step = F32(0.8) * rar.grey(frame)
    assert step.dtype == F32
    want = step + F32(0.05)
    assert np.array_equal(got[block].view(np.int32), want[block].view(np.int32))
    assert np.array_equal(got[~block].view(np.int32), rar.grey(render)[~block].view(np.int32))
    pyr = rer.target_intensity_pyramid(render, frame, rendered, filled, 0.8, 0.05, 2)
    assert [p.shape for p in pyr] == [(2, 3), (4, 6)]
    assert np.array_equal(pyr[1], got) and np.array_equal(pyr[0], rar.half(got))
    # a depth of the same value is not a replacement, whatever the colours
    assert np.array_equal(rer.composite(render, frame, rendered, rendered, 0.8, 0.05), rar.grey(render))
