"""rtgs_map_deform_sh (csrc/map_deform_sh.hip) against its definition tests/map_deform_sh_reference.py, bit for bit; the render of a
map deformed with its SH bands turned at the moved pose against the render before; MapOptimizer.deform_rows(sh_table=...)."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import sh_rotation as shr
from rtg_slam_amd import synth
from rtg_slam_amd.rgbd_align import se3_exp
from tests import map_deform_reference as mdr
from tests import map_deform_sh_reference as msr
from tests import raster_util as ru
from tests.test_map_deform_cpu import DELTA_A, DELTA_B
from tests.test_map_deform_gpu import CAM, DELTA, KEYFRAMES, N_FRAMES, bits, differing_pixels
from tests.test_sh_rotation_cpu import oracle_counts, sh_render_scene

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32


def corrections_of_a_closure():
    """The corrections behind tests/test_map_deform_gpu.py::table_of_a_closure: twenty frames, keyframes 0 (held: the identity),
    5 and 12."""
    old = [np.eye(4), se3_exp([0, 0.2, 0, 0.3, 0, 0.1]), se3_exp([0, 0.5, 0, 0.6, 0.1, 0.2])]
    new = [old[0], DELTA_A @ old[1], DELTA_B @ old[2]]
    return lc.frame_corrections(KEYFRAMES, old, new, N_FRAMES)


def sh_rows(n, seed):
    return (np.random.default_rng(seed).normal(size=(n, 16, 3)) * 0.05).astype(F32)


def run_kernel(shs, tick, sh_table):
    from rtg_slam_amd import _lib
    lib = _lib.load()
    s = torch.from_numpy(shs.copy()).to(DEV)
    t, tb = torch.from_numpy(np.ascontiguousarray(tick)).to(DEV), torch.from_numpy(np.ascontiguousarray(sh_table)).to(DEV)
    kind = {torch.int32: 0, torch.int64: 1}[t.dtype]
    rc = lib.rtgs_map_deform_sh(_lib.ptr(s), _lib.ptr(t), kind, s.shape[0], _lib.ptr(tb), tb.shape[0], _lib.stream(DEV))
    assert rc == 0
    return s.cpu().numpy()


def ticks(pattern, n, dtype, sh_table):
    rng = np.random.default_rng(n + 1)
    if pattern == "random":                                                      # mixed waves; below 0 .. beyond the table
        tick = rng.integers(-3, N_FRAMES + 6, size=n)
        pin = np.array([-2, 0, 5, 12, 3, 8, 15, 19, 20, 24, 2 ** 31 - 1 if dtype == np.int32 else 2 ** 40, -2 ** 31])
        tick[:min(n, pin.size)] = pin[:n] if n < pin.size else pin
        if n == 1:
            tick[0] = 8
    elif pattern == "runs":                                                      # ascending runs of 64 .. 150 equal ticks
        lengths = rng.integers(64, 151, size=n // 64 + 1)
        tick = np.repeat((1 + np.arange(lengths.size)) % N_FRAMES, lengths)[:n]  # frame 0 (flag 0) comes round at 5 000 rows
    else:                                                                        # alternating flag-0 and flag-1 frames
        assert sh_table[0, 83] == 0 and sh_table[1:, 83].all()
        tick = np.where(np.arange(n) % 2 == 0, 0, 1 + np.arange(n) % (N_FRAMES - 1))
    return tick.astype(dtype)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("pattern", ["random", "runs", "alternating"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 5000])
def test_bit_equal_to_the_definition(n, pattern, dtype):
    shs = sh_rows(n, seed=n)
    sh_table = shr.sh_rotation_table(corrections_of_a_closure())
    tick = ticks(pattern, n, dtype, sh_table)
    want = msr.deform_sh(shs, tick, sh_table)
    got = run_kernel(shs, tick, sh_table)
    assert np.array_equal(bits(got), bits(want))
    if n >= 63 and (pattern != "runs" or n == 5000):
        held = sh_table[np.clip(tick.astype(np.int64), 0, N_FRAMES - 1), 83] == 0
        assert held.any() and (~held).any()
        assert np.array_equal(bits(got[held]), bits(shs[held])) and not np.array_equal(bits(got[~held]), bits(shs[~held]))
    again = run_kernel(shs, tick, sh_table)                                      # two runs are bit-equal
    assert np.array_equal(bits(again), bits(got))


def test_held_rows_and_the_dc_term_are_not_written_and_refusals_launch_nothing():
    from rtg_slam_amd import _lib
    lib = _lib.load()
    n = 400
    shs = sh_rows(n, seed=9)
    shs[::3, 5] = -0.0                                                           # M x would make these +0.0
    shs[1::3] = -0.0
    shs[:, 0] = np.nan                                                           # the DC term: a NaN's payload survives only untouched
    shs[::2, 0] = -0.0
    sh_table = shr.sh_rotation_table(corrections_of_a_closure())
    sh_table[7, 83] = -0.0                                                       # compares equal to 0, whatever the blocks say
    tick = np.where(np.arange(n) % 2 == 0, 7, -1).astype(np.int32)               # frame 7's flag, and frame 0's
    tick[128:256] = 7                                                            # two whole blocks of rows that stay
    got = run_kernel(shs, tick, sh_table)
    assert np.array_equal(bits(got), bits(shs))
    tick[:] = 9
    got = run_kernel(shs, tick, sh_table)
    assert not np.array_equal(bits(got[1::3, 1:]), bits(shs[1::3, 1:]))          # the same rows ARE written once the flag is set
    assert np.array_equal(bits(got[:, 0]), bits(shs[:, 0]))                      # coefficient 0 never
    tick[64:192] = 0                                                             # held blocks between moved ones
    got = run_kernel(shs, tick, sh_table)
    assert np.array_equal(bits(got[64:192]), bits(shs[64:192])) and np.array_equal(bits(got[:, 0]), bits(shs[:, 0]))
    E = _lib.CONSTANTS["RTGS_E_INVALID"]
    s, t, tb = torch.from_numpy(shs).to(DEV), torch.from_numpy(tick).to(DEV), torch.from_numpy(sh_table).to(DEV)
    p, st = _lib.ptr, _lib.stream(DEV)
    good = [p(s), p(t), 0, n, p(tb), N_FRAMES, st]
    for i, v in ((0, None), (1, None), (4, None), (2, 2), (2, -1), (3, -1), (3, 2 ** 31), (5, 0), (5, -4),
                 (0, s.data_ptr() + 4), (0, s.data_ptr() + 8), (4, tb.data_ptr() + 8)):
        bad = list(good)
        bad[i] = v
        assert lib.rtgs_map_deform_sh(*bad) == E, (i, v)
    empty = list(good)
    empty[3] = 0
    assert lib.rtgs_map_deform_sh(*empty) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(s.cpu().numpy()), bits(shs))


# ---- render equivalence ----

def test_render_equivalence():
    """The map rendered at POSE and the deformed map - its SH bands turned by the KERNEL - rendered at DELTA POSE (3 degrees, 5
    cm, every tick) show the same picture, higher bands and all.  The CPU oracle rendering the same pair sets the scale
    (tests/test_sh_rotation_cpu.py::oracle_counts: 0 of 19 200 pixels differ by more than 1e-4 with the bands turned, 19 168 with
    the bands left as they were); the HIP renders may differ in as many, plus the 4 pixels the parity tests allow a map.  With
    the bands left, more than half of the covered pixels differ on the device as well."""
    g, d, plain, s0, s1, tick, table, sh_table = sh_render_scene()
    got = run_kernel(g["shs"].numpy(), tick.astype(np.int32), sh_table)
    assert np.array_equal(bits(got), bits(d["shs"].numpy()))                     # the kernel's rows ARE the rendered ones
    assert not np.array_equal(bits(got[:, 1:]), bits(g["shs"].numpy()[:, 1:]))
    turned = dict(d)
    turned["shs"] = torch.from_numpy(got)
    out_a, _ = ru.hip_run(s0, g)
    out_b, _ = ru.hip_run(s1, turned)
    out_c, _ = ru.hip_run(s1, plain)
    count, covered = differing_pixels(out_a, g["normal"], out_b, turned["normal"])
    left, _ = differing_pixels(out_a, g["normal"], out_c, plain["normal"])
    ref, ref_left, _ = oracle_counts()
    pixels = CAM.H * CAM.W
    print(f"render equivalence with the SH bands turned: {count} of {pixels} pixels differ by more than 1e-4 on the device, {ref} "
          f"in the oracle; with the bands left {left} on the device, {ref_left} in the oracle; {100 * covered:.1f} % covered")
    assert covered > 0.5
    assert count <= ref + 4
    assert left > 0.5 * covered * pixels


# ---- the map object ----

def _optimizer():
    from rtg_slam_amd import map_optim as mo
    g = synth.surface_gaussians(3000, CAM, seed=4)
    packed = mo.pack_from_activated({k: v.to(DEV) for k, v in g.items()})
    opt = mo.ShardedMapOptimizer(packed, n_frozen=1000, capacity=4096)
    tick = opt.add_aux("add_tick", 1, torch.int32, 0)
    tick[:3000, 0] = torch.arange(3000, dtype=torch.int32, device=DEV) % 7
    return opt, tick


def test_deform_rows_turns_the_sh_block_only_when_asked(monkeypatch):
    from rtg_slam_amd import _lib
    lib = _lib.load()
    calls = {"rtgs_map_deform": 0, "rtgs_map_deform_sh": 0}
    for name in calls:
        def counted(*a, _real=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    D = np.stack([np.eye(4)] + [DELTA] * 6)
    table = torch.from_numpy(lc.deform_table(D)).to(DEV)
    sh_table = torch.from_numpy(shr.sh_rotation_table(D)).to(DEV)
    t = (np.arange(3000) % 7).astype(np.int32)

    plain, _ = _optimizer()
    before = plain.params.cpu().numpy()
    assert np.abs(before[:, 6:51]).max() > 0                                     # the map has higher bands
    version, key = plain.version, plain.frozen_key
    plain.deform_rows(table, sh_table=None)                                      # what the call is today
    assert calls == {"rtgs_map_deform": 1, "rtgs_map_deform_sh": 0}
    bumps = (plain.version - version, plain.frozen_key != key, plain._act_valid, plain.attach_init, plain._history)
    after_plain = plain.params.cpu().numpy()
    want_x, want_r = mdr.deform(before[:, :3], before[:, 51:59], t, table.cpu().numpy())
    assert np.array_equal(bits(after_plain[:, :3]), bits(want_x)) and np.array_equal(bits(after_plain[:, 51:59]), bits(want_r))
    assert np.array_equal(bits(after_plain[:, 3:51]), bits(before[:, 3:51]))     # SH untouched

    opt, tick = _optimizer()
    assert np.array_equal(bits(opt.params.cpu().numpy()), bits(before))
    moments = {k: opt.state["shs"][k].view(torch.int32).clone() for k in ("m", "v")}
    version, key = opt.version, opt.frozen_key
    opt.deform_rows(table, sh_table=sh_table)
    assert calls == {"rtgs_map_deform": 2, "rtgs_map_deform_sh": 1}
    assert (opt.version - version, opt.frozen_key != key, opt._act_valid, opt.attach_init, opt._history) == bumps
    assert bumps[0] > 0 and bumps[1] and not bumps[2]
    after = opt.params.cpu().numpy()
    want_s = msr.deform_sh(before[:, 3:51].reshape(-1, 16, 3), t, sh_table.cpu().numpy()).reshape(-1, 48)
    assert np.array_equal(bits(after[:, 3:51]), bits(want_s))
    assert not np.array_equal(bits(after[:, 6:51]), bits(before[:, 6:51]))
    assert np.array_equal(bits(after[:, :3]), bits(after_plain[:, :3]))          # xyz and raw8 as deform_rows(table) alone gives
    assert np.array_equal(bits(after[:, 51:59]), bits(after_plain[:, 51:59]))
    assert np.array_equal(bits(after[t == 0]), bits(before[t == 0]))             # frozen and trainable rows alike
    assert all(torch.equal(opt.state["shs"][k].view(torch.int32), moments[k]) for k in moments)      # the Adam moments stay
    # a 64-bit tick array
    opt64, tick64 = _optimizer()
    opt64.deform_rows(table, tick=tick64[:, 0].long().contiguous(), sh_table=sh_table)
    assert np.array_equal(bits(opt64.params.cpu().numpy()), bits(after))
    # the refusals: shape, dtype, device, n_frames - nothing moves
    n_calls = dict(calls)
    for bad in (sh_table[:, :83].contiguous(), sh_table.double(), sh_table.cpu(), sh_table[:6].contiguous(),
                torch.cat([sh_table, sh_table[:1]]), sh_table.reshape(-1), sh_table.t().contiguous().t(), sh_table.cpu().numpy()):
        with pytest.raises(ValueError):
            opt.deform_rows(table, sh_table=bad)
    assert calls == n_calls and np.array_equal(bits(opt.params.cpu().numpy()), bits(after))
    opt.begin_global_optimization()
    with pytest.raises(RuntimeError):
        opt.deform_rows(table, sh_table=sh_table)
    opt.end_global_optimization()
