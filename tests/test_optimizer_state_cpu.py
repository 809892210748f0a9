"""The optimiser-state bookkeeping of ShardedMapOptimizer (rtg_slam_amd/map_optim.py) on the CPU, the float64 model of
tests/optimizer_model.py against the suite's own Adam restatement, the CPU pair the GPU tolerances come from, the mapper's
`gaussians_fix` skip against the same run without it, and Mapping.global_optimization leaving the global scope when the
mask renders raise."""
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from rtg_slam_amd import map_optim as mo  # noqa: E402
from rtg_slam_amd import mapping as mp  # noqa: E402
from rtg_slam_amd import synth  # noqa: E402
from tests import optimizer_model as om  # noqa: E402
from tests import test_mapping_cpu as tm  # noqa: E402
from tests import torch_doubles as td  # noqa: E402
from tests.dist_util import adam_reference  # noqa: E402
from tests.mapping_doubles import TorchOps  # noqa: E402

CAM = synth.CameraSpec(32, 48, 40.0, 40.0, 23.5, 15.5)


def _packed(n, seed):
    return mo.pack_from_activated(synth.random_gaussians(n, CAM, seed=seed))


def _opt(packed, **kw):
    return mo.ShardedMapOptimizer(packed.clone(), adam_fn=adam_reference, activate_fn=td.activate8, **kw)


def _poke(opt, rows, value=3.0):
    for n, _, _ in mo.BLOCKS:
        for k in ("m", "v", "ever"):
            opt.state[n][k][rows] = value


def _nonzero_rows(opt):
    out = set()
    for n, _, _ in mo.BLOCKS:
        for k in ("m", "v", "ever"):
            t = opt.state[n][k]
            out |= set(torch.nonzero(t.reshape(t.shape[0], -1).ne(0).any(dim=1)).reshape(-1).tolist())
    return sorted(out)


# ---------------------------------------------------------------------- _mark_adam / _zero_adam / _allocate
def test_mark_adam_keeps_the_union_and_ignores_empty_ranges():
    opt = _opt(_packed(20, 1), capacity=32)
    assert opt._adam_dirty is None
    opt._mark_adam(5, 5)                                                # empty: ignored
    opt._mark_adam(9, 4)                                                # hi < lo: ignored
    assert opt._adam_dirty is None
    opt._mark_adam(4, 9)
    assert opt._adam_dirty == (4, 9)
    opt._mark_adam(12, 15)                                              # the union is one interval: the gap is covered too
    assert opt._adam_dirty == (4, 15)
    opt._mark_adam(0, 6)
    assert opt._adam_dirty == (0, 15)
    opt._mark_adam(7, 7)
    assert opt._adam_dirty == (0, 15)


def test_all_is_sticky_until_the_clear():
    opt = _opt(_packed(20, 2), capacity=32)
    opt._mark_adam(2, 4)
    opt._adam_dirty = "all"                                             # what _adam (the autograd step) records
    opt._mark_adam(0, 1)
    assert opt._adam_dirty == "all"
    _poke(opt, [0, 17, 31])
    opt._zero_adam()
    assert opt._adam_dirty is None and _nonzero_rows(opt) == []
    opt.step(lambda gd: gd["xyz"].pow(2).sum() + gd["shs"].sum() + gd["scales"].sum())
    assert opt._adam_dirty == "all" and _nonzero_rows(opt) != []
    opt.begin_local_optimization()
    assert opt._adam_dirty is None and _nonzero_rows(opt) == [] and opt.step_count == 0


def test_zero_adam_clears_the_recorded_rows_and_only_those():
    """Poked rows inside the recorded range are cleared; a poked row OUTSIDE it survives - which is the failure an unmarked
    writer causes, and shows that this test can see it."""
    opt = _opt(_packed(20, 3), capacity=32)
    opt._mark_adam(3, 11)
    _poke(opt, [3, 7, 10])
    _poke(opt, [11, 25])                                                # written without a mark
    opt._zero_adam()
    assert _nonzero_rows(opt) == [11, 25] and opt._adam_dirty is None
    opt._zero_adam()                                                    # nothing recorded: nothing cleared
    assert _nonzero_rows(opt) == [11, 25]
    opt._mark_adam(11, 12)
    opt._zero_adam()
    assert _nonzero_rows(opt) == [25]


def test_zero_adam_clamps_the_range_at_the_array_length():
    opt = _opt(_packed(20, 4), capacity=32)
    rows = opt.state["xyz"]["m"].shape[0]
    assert rows == 32
    opt._mark_adam(28, 10_000)
    _poke(opt, [28, 31])
    _poke(opt, [27])
    opt._zero_adam()
    assert _nonzero_rows(opt) == [27]


def test_allocate_carries_the_moments_and_the_recorded_range_stays_valid():
    a, b = _packed(20, 5), _packed(30, 6)
    opt = _opt(a, n_frozen=4, capacity=24)
    opt._mark_adam(0, 16)
    for n, c0, c1 in mo.BLOCKS:
        opt.state[n]["m"][:16] = torch.arange(16.0).reshape(16, 1) + 1.0
        opt.state[n]["v"][:16] = 0.5
        opt.state[n]["ever"][:16] = 1
    steps = opt.total_steps
    opt.append_rows(b)                                                  # 50 > 24: _allocate(50)
    assert opt.capacity >= 50 and opt.state["xyz"]["m"].shape[0] >= 50
    assert opt._adam_dirty == (0, 16) and opt.total_steps == steps
    for n, c0, c1 in mo.BLOCKS:
        assert torch.equal(opt.state[n]["m"][:16, 0], torch.arange(16.0) + 1.0)
        assert float(opt.state[n]["v"][:16].min()) == 0.5 and int(opt.state[n]["ever"][:16].sum()) == 16
        assert int(opt.state[n]["m"][16:].count_nonzero()) == 0 and int(opt.state[n]["ever"][16:].count_nonzero()) == 0
    opt._zero_adam()                                                    # the range recorded BEFORE the re-allocation clears the new arrays
    assert _nonzero_rows(opt) == []


def test_begin_restarts_the_step_counter_and_the_rates_but_never_total_steps():
    a = _packed(12, 7)
    w = torch.linspace(0.5, 1.5, 64)
    loss = lambda gd: (gd["xyz"] * w[:gd["xyz"].shape[0], None]).pow(2).sum() + gd["shs"].sum()
    opt = _opt(a, n_frozen=5)
    for _ in range(3):
        opt.step(loss)
    assert (opt.step_count, opt.total_steps) == (3, 3)
    opt.begin_local_optimization()
    assert (opt.step_count, opt.total_steps) == (0, 3)
    opt.begin_global_optimization(mo.global_lr_scale(final=False))
    assert opt._lr("xyz").abs().max() == 0 and (opt.step_count, opt.total_steps) == (0, 3)
    opt.step(loss)
    opt.end_global_optimization()
    assert opt._lr_scope is None and torch.equal(opt._lr("xyz"), opt.state["xyz"]["lr"]) and opt.total_steps == 4
    opt.append_rows(_packed(40, 8))                                     # re-allocates
    assert opt.total_steps == 4
    opt.step(loss)
    assert (opt.step_count, opt.total_steps) == (1, 5)                  # end_global left a stale state: the step started over


# ---------------------------------------------------------------------- AdamModel and the CPU pair
def test_adam_model_equals_the_adam_restatement_over_50_steps():
    """AdamModel's row rule (a row is stepped once it has carried gradient) leaves exactly what dense Adam leaves: for a row
    that never had gradient dense Adam computes m = v = 0 and an update of 0.  tests.dist_util.adam_reference in float64,
    dense, against the model over 50 steps of gradients with zeros, idle rows and eight decades of magnitude."""
    n = 120
    lr = mo.default_lr_columns()
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, om.COLS, generator=gen)
    p0[:, 51] = 4.595
    model = om.AdamModel(p0, 0, lr)
    model.begin_local()
    model.snapshot = None
    p, m, v = p0.double().clone(), torch.zeros(n, om.COLS, dtype=torch.float64), torch.zeros(n, om.COLS, dtype=torch.float64)
    for t, (g, on) in enumerate(om.synthetic_gradients(n, 50, seed=9), start=1):
        model.step(g[:, 0:3], g[:, 3:51], g[:, 51:59], on)
        adam_reference(p, g.double(), m, v, lr.double(), t, om.EPS)
        assert model.step_count == t
        assert float((model.p - p).abs().max()) <= 1e-13 and float((model.m - m).abs().max()) <= 1e-15
    assert float((p - p0.double()).abs().max()) > 1e-3
    never = ~model.ever.any(dim=1)
    assert torch.equal(model.p[never], p0.double()[never])


def test_adam_model_attach_term_is_the_gradient_of_the_regulariser():
    """The xyz part of the attach gradient (mapper.py:384-401): d/dxyz of 1000 mean((xyz - xyz0)[selected]^2), by autograd,
    for the rows the kernels look at (those that carry gradient or were stepped)."""
    n = 40
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, om.COLS, generator=gen)
    p0[:, 51] = torch.where(torch.arange(n) % 3 == 0, torch.tensor(-2.197), torch.tensor(4.595))      # opacity 0.1 / 0.99
    lr = mo.default_lr_columns()
    model = om.AdamModel(p0, 10, lr)
    model.begin_local()
    assert int(model.snapshot["sel"].sum()) == int((torch.arange(10, n) % 3 == 0).sum())
    on = torch.ones(n - 10, dtype=torch.bool)
    z = lambda c: torch.zeros(n - 10, c)
    model.step(torch.ones(n - 10, 3) * 1e-3, z(48), z(8), on)            # every row moves away from its snapshot
    x = model.p[10:, 0:3].clone().requires_grad_(True)
    sel = model.snapshot["sel"]
    (1000 * ((x[sel] - model.snapshot["p"][sel, 0:3]) ** 2).mean()).backward()
    before, m_before = model.p.clone(), model.m.clone()
    model.step(z(3), z(48), z(8), torch.zeros(n - 10, dtype=torch.bool))   # no render gradient: the attach term alone
    g = (model.m[:, 0:3] - om.B1 * m_before[:, 0:3]) / (1 - om.B1)
    assert float((g - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max()) and float(x.grad[sel].abs().min()) > 0
    assert torch.equal(model.p[:10], before[:10])


def test_cpu_figures_the_gpu_tolerances_are_derived_from():
    """adam1 restated in float32 (adam_common.h's operation order, no fused multiply-add) against AdamModel on 50 steps of
    synthetic gradients: the largest deviation per step taken, the largest one-step identity residual and the largest
    distance of m^2 / v from 10 stay at or under the figures recorded in tests/optimizer_model.py - and are not far below
    them, so the recorded figures are what this pair gives.  The stream draws 1e-5 of its elements below 1e-17 (the one
    exclusion of the GPU comparison): 3.0e-4 of the stepped elements meet one within their 50 steps, bound 0.1 %."""
    fig = om.measure_cpu_figures()
    print(fig)
    assert 0.5 * om.CPU_DEVIATION_UNITS <= fig["deviation"] <= om.CPU_DEVIATION_UNITS
    assert 0.5 * om.CPU_IDENTITY_UNITS <= fig["identity"] <= om.CPU_IDENTITY_UNITS
    assert 0.5 * om.CPU_RATIO_REL <= fig["ratio"] <= om.CPU_RATIO_REL
    assert fig["tiny_share"] <= 1e-3
    # a stale moment or a step counter that is off by one is hundreds of times 4 x the figure, even at |p| = 0.5
    lr = mo.default_lr_columns().numpy()
    p, g = np.float32(0.5), np.float32(1e-3)
    good, _, _ = om.adam1_f32(p, g, np.float32(0), np.float32(0), lr[0], 1)
    stale, _, _ = om.adam1_f32(p, g, np.float32(-1e-4), np.float32(1e-8), lr[0], 1)
    late, _, _ = om.adam1_f32(p, g, np.float32(0), np.float32(0), lr[0], 2)
    u = om.unit(good, lr[0])
    assert abs(float(stale) - float(good)) / u > 100 * om.KERNEL_FACTOR * om.CPU_DEVIATION_UNITS
    assert abs(float(late) - float(good)) / u > 100 * om.KERNEL_FACTOR * om.CPU_DEVIATION_UNITS


# ---------------------------------------------------------------------- the mapper's skip, on the CPU
def _run_changing(skip):
    args = tm._args()
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(3)
    ops = TorchOps(args)
    m = mp.Mapping(args, torch.device("cpu"), ops=ops, capacity=300)
    o = m.opt
    seen = dict(steps=0, skipped=0, looked=0)
    ops_step, fix = ops.step, m.gaussians_fix

    def step(*a, **k):
        before = o.total_steps
        out = ops_step(*a, **k)
        seen["steps"] += 1
        assert o.total_steps == before + 1 == seen["steps"]
        return out
    ops.step = step

    def gaussians_fix(mask=None):
        if not skip:
            m.__dict__.pop("_fix_seen_steps", None)
        elif mask is None and o.n_train > 0:
            if o.total_steps == getattr(m, "_fix_seen_steps", None):
                seen["skipped"] += 1
                conf_u = m.aux("confidence", "unstable").reshape(-1)
                assert int((conf_u > args.stable_confidence_thres).sum()) == 0
            else:
                seen["looked"] += 1
        return fix(mask)
    m.gaussians_fix = gaussians_fix
    frames, capacities = [], set()
    for fid, (d, c, c2w) in enumerate(tm._changing_stream(15)):
        fr = mp.Frame(tm.CAM, c2w, torch.device("cpu"), uid=fid)
        m.mapping(fr, tm._frame_map(d, c, fr, args), fid)
        m.get_render_output(fr)
        assert o.total_steps == seen["steps"]                            # never reset: not by a begin, an append or _allocate
        capacities.add(o.capacity)
        frames.append((o.params.clone(), o.n_frozen, m.stats["fixed"]))
        m.time += 1
    return frames, seen, capacities, m


def test_the_fix_skip_changes_nothing_over_the_changing_stream():
    """The CPU double of the GPU check: the 15-frame changing stream of tests/test_mapping_cpu.py (releases, a large fix) with
    the skip and with `_fix_seen_steps` deleted before every call - parameters, n_frozen and the number of fixed Gaussians
    are equal after every frame; at every early return no unstable Gaussian is over the threshold."""
    with_skip, seen, capacities, m = _run_changing(True)
    without, _, _, _ = _run_changing(False)
    assert seen["skipped"] > 0 and seen["looked"] > 0 and seen["steps"] > 0 and m.stats["fixed"] > 0
    assert len(capacities) > 1                                          # the map was re-allocated on the way
    assert len(with_skip) == len(without) == 15
    for fid, (a, b) in enumerate(zip(with_skip, without)):
        assert a[1] == b[1] and a[2] == b[2], fid
        assert torch.equal(a[0], b[0]), fid


# ---------------------------------------------------------------------- global_optimization leaves its scope
class _MaskRenderFailed(RuntimeError):
    pass


def test_global_optimization_leaves_the_global_scope_when_the_mask_render_raises():
    """Mapping.global_optimization opens its try directly behind begin_global_optimization(): an exception in
    evaluate_render_range (before the first step) propagates as it is, and the map is back in the local scope - appends
    and a new local optimisation work."""
    args = tm._args()
    m, ops, log = tm._run(3, args)
    o = m.opt
    assert o.n_frozen > 0 and m.get_keyframe_num > 0 and o._scope == "local"
    err = _MaskRenderFailed("mask render")

    def boom(*a, **k):
        assert o._scope == "global"
        raise err
    m.evaluate_render_range = boom
    with pytest.raises(_MaskRenderFailed) as info:
        m.global_optimization(select_keyframe_num=args.global_keyframe_num)
    assert info.value is err
    assert o._scope == "local" and o._lr_scope is None and m.iter == 0
    n = o.N
    o.append_rows(o.params[:2].clone())
    assert o.N == n + 2
    o.begin_local_optimization()
    assert o.step_count == 0 and o.attach_init is not None and o.attach_init["xyz"].shape[0] == o.n_train

    # the ORIGINAL exception survives a failing end_global_optimization() too
    o.begin_local_optimization()
    end = o.end_global_optimization

    def failing_end():
        end()
        raise RuntimeError("end failed")
    o.end_global_optimization = failing_end
    with pytest.warns(RuntimeWarning, match="end failed"):              # ... which is reported, not dropped
        with pytest.raises(_MaskRenderFailed) as info:
            m.global_optimization(select_keyframe_num=args.global_keyframe_num)
    assert info.value is err and o._scope == "local"
    if hasattr(err, "__notes__"):
        assert any("end failed" in n for n in err.__notes__)
