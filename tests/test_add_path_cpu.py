"""The replay harness of tests/add_path_replay.py on the CPU: torch doubles on both sides (FusedTorchOps - TorchOps plus doubles of
the fused calls, so Mapping's fused branches run - against TorchOps through the tensor branches).  It has to pass trivially, it has
to show that every frame of both streams was compared, and it has to FAIL when a double is made subtly wrong."""
import pytest
import torch

from tests import add_path_replay as rp, margins, test_mapping_cpu as tm
from tests.mapping_doubles import TorchOps
from rtg_slam_amd import mapping as mp

CPU = torch.device("cpu")


def _replay(n_frames, changing=False, args=None, seed=0, **switches):
    args = args if args is not None else tm._args()
    ops = rp.FusedTorchOps(args, seed=seed)
    for k, v in switches.items():
        assert hasattr(ops, k)
        setattr(ops, k, v)
    m = mp.Mapping(args, CPU, ops=ops, capacity=600)
    ops.opt_of = lambda: m.opt
    r = rp.Replay(m, TorchOps(args))
    seen = r.run((tm._changing_stream if changing else tm._stream)(n_frames), tm.CAM, rp.frame_maps(CPU))
    return r, seen


def check_not_vacuous(seen, n_frames, changing):
    """Every frame was compared, and every kind of decision occurred at least once over the two streams' frames."""
    assert seen["frames"] == n_frames and seen["books"] == n_frames and seen["adds"] >= (12 if changing else 6), seen
    assert seen["rows"] > 0 and seen["filter_drop"] >= 1 and seen["attach"] >= 1 and seen["del_unstable"] >= 1, seen
    if changing:
        assert seen["release"] >= 1 and seen["del_stable"] >= 1, seen


@pytest.mark.parametrize("n_frames,changing", [(7, False), (15, True)])
def test_fused_doubles_equal_the_tensor_form_on_every_frame(n_frames, changing):
    r, seen = _replay(n_frames, changing)
    print(seen)
    check_not_vacuous(seen, n_frames, changing)
    assert r.render_checked and seen["act_max_diff"] == 0.0
    margins.record("add_path", frames=seen["frames"], rows_added=seen["rows"], rows_bookkeeping=seen["rows_bookkeeping"],
                   rows_excused_mean_band=seen["excused"])


def test_a_filter_ratio_of_0_61_is_caught():
    """Only a candidate whose distance lies in [0.6, 0.61) of a neighbour's radius sees the difference - about one in a thousand
    of this stream's 1 400.  The seed of the double's draw is one under which the stream has such a candidate (frame 2); the
    control with the right ratio passes under the same seed."""
    _replay(7, seed=1)
    with pytest.raises(AssertionError, match="filter decision differs"):
        _replay(7, seed=1, filter_ratio=0.61)


def test_an_existing_gaussian_index_off_by_one_row_is_caught():
    with pytest.raises(AssertionError, match="accepted|raw scales"):
        _replay(7, new_rows_shift=1)


def test_a_stale_stable_structure_is_caught():
    """Control first: routed through knn_stable (rebuilt when frozen_key changes) the stream passes and the structure IS rebuilt
    after a freeze; the same double without the rebuild fails."""
    r, seen = _replay(7, route_stable=True)
    assert r.f.ops.stable_calls >= 5 and 2 <= r.f.ops.stable_builds <= r.f.ops.stable_calls, (r.f.ops.stable_calls, r.f.ops.stable_builds)
    with pytest.raises(AssertionError, match="accepted|raw scales|surviving|existing row"):
        _replay(7, route_stable=True, stale_stable=True)


def test_the_float64_mean_band_of_the_delete_reference():
    """delete_reference: rows far from 10 x mean are decided, a row AT 10 x mean lies in the band, an old row never does."""
    n = 1000
    sc = torch.full((n, 3), 0.01)
    sc[5] = 0.5                                                         # a giant: radius 0.5 against 10 x mean ~ 0.105
    tick = torch.zeros(n, 1, dtype=torch.int32)
    tick[7] = -100
    want, band, thr = rp.delete_reference(sc, tick, 10, 50)
    assert bool(want[5]) and bool(want[7]) and int(want.sum()) == 2 and int(band.sum()) == 0
    sc[9] = float(thr) * (n / (n - 10.0))                               # moves the mean with it: solve r = 10 (sum' + r) / n
    r9 = 10.0 * float(rp.radius32(sc).double().sum() - rp.radius32(sc)[9].double()) / (n - 10.0)
    sc[9] = r9
    want, band, thr = rp.delete_reference(sc, tick, 10, 50)
    assert abs(r9 - thr) <= 1e-6 * thr and bool(band[9]) and int(band.sum()) == 1 and not bool(band[7])
