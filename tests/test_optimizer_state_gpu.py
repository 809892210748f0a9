"""The lazily cleared optimiser state of ShardedMapOptimizer (rtg_slam_amd/map_optim.py) against a float64 Adam model.

"A fresh Adam" is a partial clear of the rows recorded as dirty: `_adam_dirty` (`_mark_adam` / `_zero_adam`),
`RowGradArena._dirty` (widened by the `train` setter), `_stale` with `_clean()`, and `_allocate()`, which carries moments
across a reallocation.  The clears are right only if every writer of those arrays marks its rows and if `step_count`, the
learning-rate scope and the snapshot restart with the scope.  Here one small map goes through every transition the product
makes (`_schedule`), under both tails, and

(a) the state invariants are asserted EXACTLY after every operation (`_Driver.check_*`, on the full allocated arrays);
(c) with the three-kernel tail, which leaves the step's gradient rows in the arena, tests/optimizer_model.py `AdamModel`
    is fed those rows and must land where the product lands (teacher forcing: slot order and the signs of ~0 gradients are
    out of the comparison);
(d) with the fused tail, which keeps gradients in registers, two gradient-free identities are evaluated in float64 on the
    product's own m, v, p;
(e) the mapper's `gaussians_fix` skip (`total_steps == _fix_seen_steps`) is checked against what the skipped body would
    have computed.

No tolerance here is relative to another run of the code under test: each is exact or a multiple of a figure measured
on the CPU between a float32 restatement of adam1 and the float64 model (tests/test_optimizer_state_cpu.py)."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import synth
from tests import margins
from tests import optimizer_model as om
from tests import raster_util as ru

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAM = synth.CameraSpec(128, 192, 160.0, 160.0, 95.5, 63.5)          # the camera of tests/test_trainable_gpu.py
POOL, N0, NF0, CAP0 = 6000, 3000, 1000, 3500                        # one append of 400 fits, the later ones re-allocate
WIDTH = torch.tensor([3, 48, 8])


def _setup():
    from rtg_slam_amd import map_optim as mo
    g, s = ru.make_scene(POOL, CAM, seed=4, pose_seed=2)             # opacities 0.99 or 0.1: far from the attach test's 0.9
    pool = mo.pack_from_activated({k: v.to(DEV) for k, v in g.items()})
    gen = torch.Generator().manual_seed(4)
    gt_c = torch.rand(3, CAM.H, CAM.W, generator=gen).to(DEV)
    gt_d = (1.0 + torch.rand(1, CAM.H, CAM.W, generator=gen)).to(DEV)
    return mo, pool, ru.hip_settings(s, DEV), gt_c, gt_d


def _nz_rows(t):
    """Indices of the rows of `t` that hold a non-zero."""
    return torch.nonzero(t.reshape(t.shape[0], -1).ne(0).any(dim=1)).reshape(-1)


def _inside(rows, rng):
    if rows.numel() == 0 or rng == "all":
        return True
    return rng is not None and int(rows.min()) >= rng[0] and int(rows.max()) < rng[1]


class _Driver:
    """Runs operations on the product (and on the model, mode "teacher"), and checks after each one.  `mode`: None = the
    exact invariants (a), "teacher" = (c), "identity" = (d).  The invariants look at the bookkeeping itself (`_adam_dirty`,
    `_dirty`, `_lr_scope`, `step_count`); (c) and (d) run without them, so that they stand on their numbers alone."""

    def __init__(self, tail_mode, mode=None):
        self.mo, self.pool, self.rs, self.gt_c, self.gt_d = _setup()
        mo = self.mo
        self.mode = mode
        self.opt = mo.ShardedMapOptimizer(self.pool[:N0].clone(), n_frozen=NF0, capacity=CAP0)
        self.opt.tail_mode = tail_mode
        for name, dtype, fill in (("confidence", torch.float32, 0.0), ("add_tick", torch.int32, 0),
                                  ("depth_error_counter", torch.int32, 0), ("color_error_counter", torch.int32, 0)):
            self.opt.add_aux(name, 1, dtype, fill)                   # the side arrays Mapping adds
        self.rm = torch.ones(CAM.H, CAM.W, dtype=torch.uint8, device=DEV)
        self.lr_base = mo.default_lr_columns()
        self.lr = self.lr_base.clone()                               # float32 [59]: what the scope's rates have to be
        self.t = 0                                                   # steps since the scope's begin, counted here
        self.total = 0                                               # step / step_slam calls ever
        self.p_begin = self.opt.params.clone()
        self.model = om.AdamModel(self.pool[:N0], NF0, self.lr_base) if mode == "teacher" else None
        self.worst = dict(deviation=0.0, identity=0.0, ratio=0.0)
        self.n_excluded = self.n_stepped = self.n_steps = self.n_first = 0
        self.allocations = 0
        self.moved_xyz_moments_in_global = False
        self.grad_log = []
        self.lazy_cleans = self.lazy_cleans_in_steps = 0
        self.in_steps = False
        if mode is None:
            # the product's own lazy clean is OBSERVED, never called from here: when step / step_slam / _begin run _clean()
            # on a stale state, everything has to be zero the moment it returns.  (c) and (d) run without even this wrapper:
            # there a missing lazy clean shows as a stale moment or a wrong t.
            clean = self.opt._clean

            def _clean():
                stale = bool(getattr(self.opt, "_stale", False))
                clean()
                if stale:
                    self.lazy_cleans += 1
                    self.lazy_cleans_in_steps += int(self.in_steps)
                    assert not self.opt._stale
                    self.check_all_zero("_clean")
            self.opt._clean = _clean

    # ------------------------------------------------------------------ (a) exact invariants
    def check_all_zero(self, what):
        if self.mode is not None:
            return
        o, a = self.opt, self.opt.grad_rows
        for n, _, _ in self.mo.BLOCKS:
            for k in ("m", "v", "ever"):
                assert int(o.state[n][k].count_nonzero()) == 0, (what, n, k)
        for k, t in a._full.items():
            assert int(t.count_nonzero()) == 0, (what, k)
        assert int(a._state_full.count_nonzero()) == 0 and int(a.scratch.count_nonzero()) == 0, what
        assert o.step_count == 0, what

    def check_after_step(self, what, before):
        if self.mode is not None:
            return
        o, a = self.opt, self.opt.grad_rows
        assert o.step_count == self.t, (what, o.step_count, self.t)
        nat = o.n_active_train
        N, t0 = o._active()
        assert a.train == (t0, N), what
        state = a._state_full
        for k, t in a._full.items():
            assert int(t[:t0].count_nonzero()) == 0 and int(t[N:].count_nonzero()) == 0, (what, k, "outside train")
            if k != "d_raw8":
                assert int(t[state != 1].count_nonzero()) == 0, (what, k, "row state")
            assert _inside(_nz_rows(t), a._dirty), (what, k, a._dirty)
        assert int(state[:t0].count_nonzero()) == 0 and int(state[N:].count_nonzero()) == 0, what
        now = o.params
        for bi, (n, c0, c1) in enumerate(self.mo.BLOCKS):
            st = o.state[n]
            ever = st["ever"]
            assert int(ever.max()) <= 1, (what, n)
            for k in ("m", "v", "ever"):
                assert int(st[k][nat:].count_nonzero()) == 0, (what, n, k, "beyond the active rows")
                assert _inside(_nz_rows(st[k]), o._adam_dirty), (what, n, k, o._adam_dirty)
            moved = (st["m"].ne(0) | st["v"].ne(0)).any(dim=1)
            assert not bool((moved & (ever == 0)).any()), (what, n, "moments without ever")
            idle = ever[:nat] == 0
            assert torch.equal(now[t0:N, c0:c1][idle], self.p_begin[t0:N, c0:c1][idle]), (what, n, "an unstepped row moved")
        # frozen rows (local scope) / the unstable suffix (global scope): bit for bit
        assert torch.equal(now[:t0], before[:t0]) and torch.equal(now[N:], before[N:]), what
        if float(self.lr[0:3].abs().max()) == 0.0:                   # position rate 0: xyz stands still while its moments move
            assert torch.equal(now[:, 0:3], before[:, 0:3]), what
            self.moved_xyz_moments_in_global |= bool(o.state["xyz"]["m"].ne(0).any())

    # ------------------------------------------------------------------ transitions
    def _lazy_restart(self):
        self.t = 0
        self.lr = self.lr_base.clone()

    def _adam_state(self):
        return {(n, k): self.opt.state[n][k].clone() for n, _, _ in self.mo.BLOCKS for k in ("m", "v", "ever")}

    def check_after_shape_op(self, kind, adam_before, nat_before, stale_before):
        """(a) after an operation that is neither a begin nor a step.  An append keeps what is there - the carried rows'
        m / v / ever bit for bit, also through a re-allocation - and the new rows start from zero, in the moments and in the
        arena; a history merge leaves the state alone; a permutation and the end of a global optimisation must leave the lazy
        clean pending."""
        if self.mode is not None:
            return
        o, a = self.opt, self.opt.grad_rows
        nat = o.n_active_train
        if kind in ("remove", "freeze", "end_global"):
            assert o._stale, kind
            return
        assert bool(getattr(o, "_stale", False)) == stale_before, kind
        for (n, k), old in adam_before.items():
            t = o.state[n][k]
            keep = min(nat_before, nat)
            assert torch.equal(t[:keep], old[:keep]), (kind, n, k, "carried rows")
            if not stale_before:                                     # (a pending lazy clean may still hold rows of the scope before)
                assert int(t[keep:].count_nonzero()) == 0, (kind, n, k, "new rows / beyond the active rows")
        if kind == "append" and not stale_before:
            N, t0 = o._active()
            assert a.train == (t0, N) and a.P == N, kind
            for k, t in a._full.items():
                assert int(t[t0 + nat_before:].count_nonzero()) == 0, (kind, k, "arena rows of the new rows")
            assert int(a._state_full[t0 + nat_before:].count_nonzero()) == 0, kind

    def _after_shape_op(self, kind, before, apply_to_model):
        self.p_begin = self.opt.params.clone()
        if self.model is not None:
            self.model.rebase(before)
            apply_to_model(self.model)
            assert torch.equal(self.model.p.float(), self.p_begin.cpu()), kind
            assert self.model.n_frozen == self.opt.n_frozen
            self.model.rebase(self.p_begin)

    def begin_local(self, with_confidence=False):
        o = self.opt
        self.conf = None
        if with_confidence:
            gen = torch.Generator().manual_seed(1)
            self.conf = torch.randint(1, 30, (o.n_train,), generator=gen).float().to(DEV)
        o.begin_local_optimization(confidence=self.conf)
        self._lazy_restart()
        self.check_all_zero("begin_local")
        assert o._scope == "local" and (self.mode is not None or o._lr_scope is None)
        self.p_begin = o.params.clone()
        if self.model is not None:
            self.model.begin_local(self.p_begin, self.conf)

    def begin_global(self, lr_scale):
        o = self.opt
        o.begin_global_optimization(lr_scale)
        self.t = 0
        self.lr = self.lr_base.clone() if lr_scale is None else self.lr_base * lr_scale.float()
        self.conf = None
        self.check_all_zero("begin_global")
        self.p_begin = o.params.clone()
        if self.model is not None:
            self.model.begin_global(lr_scale, self.p_begin)

    def end_global(self):
        self.opt.end_global_optimization()
        self.check_after_shape_op("end_global", None, None, None)
        self._lazy_restart()
        self.conf = None
        self.p_begin = self.opt.params.clone()
        if self.model is not None:
            self.model.end_global()

    def append(self, lo, hi, masked=False):
        o = self.opt
        before, cap = o.params.clone(), o.capacity
        pre = (self._adam_state(), o.n_active_train, bool(getattr(o, "_stale", False)))
        rows = self.pool[lo:hi].clone()
        if masked:
            valid = (torch.arange(hi - lo, device=DEV) % 4) != 1
            m = o.append_rows_masked(rows, valid, aux={"add_tick": 3})
            rows = rows[valid]
            assert m == rows.shape[0]
        else:
            o.append_rows(rows, aux={"add_tick": 3})
        self.allocations += int(o.capacity != cap)
        self.check_after_shape_op("append", *pre)
        self.conf = None                                             # sized for the rows before
        self._after_shape_op("append", before, lambda md: md.append(rows))
        return o.capacity != cap

    def remove(self, mask, start=0):
        before = self.opt.params.clone()
        self.opt.remove_rows(mask, start=start)
        self.check_after_shape_op("remove", None, None, None)
        self._lazy_restart()
        self.conf = None
        self._after_shape_op("remove", before, lambda md: md.remove(mask))

    def freeze(self, mask):
        before = self.opt.params.clone()
        self.opt.freeze_rows(mask)
        self.check_after_shape_op("freeze", None, None, None)
        self._lazy_restart()
        self.conf = None
        self._after_shape_op("freeze", before, lambda md: md.freeze(mask))

    def history_merge(self):
        o = self.opt
        before = o.params.clone()
        pre = (self._adam_state(), o.n_active_train, bool(getattr(o, "_stale", False)))
        o.history_merge(self.conf, 0.5)
        self.check_after_shape_op("history_merge", *pre)
        after = o.params.clone()
        if self.model is not None:
            self.model.rebase(before)
            self.model.history_merge(self.conf, 0.5)
            want = self.model.p.float()
            a = after.cpu()
            # the bounds tests/test_trainable_gpu.py pins the merge kernel to
            assert torch.allclose(a[:, 0:51], want[:, 0:51], atol=1e-6) and torch.allclose(a[:, 51:59], want[:, 51:59], atol=2e-6)
            self.model.rebase(after)
        self.p_begin = after

    # ------------------------------------------------------------------ steps
    def steps(self, k, autograd=False):
        o = self.opt
        for _ in range(k):
            N, t0 = o._active()
            if self.conf is None or self.conf.numel() != N - t0:
                self.conf = torch.zeros(N - t0, device=DEV)
            before = o.params.clone()
            old = {n: {k2: o.state[n][k2][:N - t0].clone() for k2 in ("m", "v", "ever")} for n, _, _ in self.mo.BLOCKS}
            if getattr(o, "_stale", False):
                # a lazy clean is pending: this step opens a new scope, in which no row has been stepped yet - what the arrays
                # still hold is the scope before, and the step itself has to get rid of it
                for n in old:
                    old[n]["ever"].zero_()
            total = o.total_steps
            self.in_steps = True
            if autograd:
                o.step(self._loss_fn())
            else:
                o.step_slam(self.rs, self.gt_c, self.gt_d, None, render_mask=self.rm, confidence=self.conf)
            self.in_steps = False
            self.t += 1
            self.total += 1
            self.n_steps += 1
            assert o.total_steps == total + 1 == self.total, (o.total_steps, total, self.total)
            self.check_after_step(f"step {self.n_steps}", before)
            if self.mode == "teacher":
                self._teacher_step(before)
            elif self.mode == "identity" and not autograd:
                self._identity_step(before, old)

    def _loss_fn(self):
        from diff_gaussian_rasterization_depth import GaussianRasterizer
        rast = GaussianRasterizer(raster_settings=self.rs)

        def loss_fn(gd):
            out = rast(means3D=gd["xyz"], opacities=gd["opacity"], shs=gd["shs"], colors_precomp=None, scales=gd["scales"],
                       rotations=gd["rotations"], cov3D_precomp=None, normal_w=gd["normal"], tile_mask=None,
                       grad_rows=gd.get("grad_rows"))
            return self.mo.slam_losses_hip(out, self.gt_c, self.gt_d, render_mask=self.rm)
        return loss_fn

    def _expanded_ever(self, N, t0):
        return torch.stack([self.opt.state[n]["ever"][:N - t0] for n, _, _ in self.mo.BLOCKS], dim=1).bool().cpu()

    def _teacher_step(self, before):
        """(c): the step's gradient rows are still in the arena (map_step.hip runs front, then rtgs_map_tail_rows_marked, and
        nothing after it; the autograd step leaves them there too) - feed them to the model, compare every active element."""
        o, a, md = self.opt, self.opt.grad_rows, self.model
        N, t0 = o._active()
        assert md.rows() == (t0, N) and md.step_count == self.t - 1
        assert float((md.lr.float() - self.lr).abs().max()) == 0.0
        has = a._state_full[t0:N] == 1
        live = md.step(a.d_means[t0:N], a.d_shs[t0:N], a.d_raw8[t0:N], has)
        assert torch.equal(md.ever, self._expanded_ever(N, t0)), "the model and the product step different rows"
        got = o.params[t0:N].cpu().double().numpy()
        want = md.p[t0:N].numpy()
        taken = md.steps_taken.numpy()
        excl = md.tiny.numpy()
        u = om.unit(got, self.lr.double().numpy()[None, :])
        dev = np.abs(got - want) / (u * np.maximum(taken, 1))
        assert float(dev[taken == 0].max(initial=0.0)) == 0.0, "an element the model does not step moved"
        ok = (taken > 0) & ~excl
        worst = float(dev[ok].max(initial=0.0))
        self.worst["deviation"] = max(self.worst["deviation"], worst)
        self.n_excluded += int((live.numpy() & excl).sum())
        self.n_stepped += int(live.sum())
        g = torch.cat([a.d_means[t0:N][has].reshape(-1), a.d_shs[t0:N][has].reshape(-1), a.d_raw8[t0:N][has].reshape(-1)]).abs().cpu()
        self.grad_log.append((int(g.numel()), int((g == 0).sum()), float(g[g > 0].min()) if bool((g > 0).any()) else 0.0, float(g.max()) if g.numel() else 0.0))
        print(f"step {self.n_steps}: t {self.t}, stepped elements {int(live.sum())}, deviation {worst:.3f} units "
              f"(bound {om.KERNEL_FACTOR * om.CPU_DEVIATION_UNITS}), excluded {int((live.numpy() & excl).sum())}")
        assert worst <= om.KERNEL_FACTOR * om.CPU_DEVIATION_UNITS, (self.n_steps, self.t, worst)

    def _identity_step(self, before, old):
        """(d): from the product's own m, v, p before and after the step, in float64."""
        o = self.opt
        N, t0 = o._active()
        n = N - t0
        cat = lambda key, src: torch.cat([src[nm][key][:n].reshape(n, -1) for nm, _, _ in self.mo.BLOCKS], dim=1).cpu().double().numpy()
        m_new, v_new = cat("m", o.state), cat("v", o.state)
        ever_new = self._expanded_ever(N, t0).repeat_interleave(WIDTH, dim=1).numpy()
        ever_old = torch.stack([old[nm]["ever"] for nm, _, _ in self.mo.BLOCKS], dim=1).bool().cpu().repeat_interleave(WIDTH, dim=1).numpy()
        p_old = before[t0:N].cpu().double().numpy()
        p_new = o.params[t0:N].cpu().double().numpy()
        lr = self.lr.double().numpy()[None, :]
        assert np.array_equal(p_new[~ever_new], p_old[~ever_new])
        want = om.expected_update(p_old, m_new, v_new, lr, self.t)
        dev = np.abs(p_new - want) / om.unit(p_new, lr)
        worst = float(dev[ever_new].max(initial=0.0))
        first = ever_new & ~ever_old & (v_new >= float(np.finfo(np.float32).tiny))
        if self.t == 1:
            assert not ever_old.any(), "a row counted as stepped before the scope's first step"
        ratio = float(np.abs(m_new[first] ** 2 / v_new[first] / 10.0 - 1.0).max(initial=0.0))
        self.worst["identity"] = max(self.worst["identity"], worst)
        self.worst["ratio"] = max(self.worst["ratio"], ratio)
        self.n_stepped += int(ever_new.sum())
        self.n_first += int(first.sum())
        print(f"step {self.n_steps}: t {self.t}, stepped {int(ever_new.sum())}, first-stepped {int(first.sum())}, identity {worst:.3f} "
              f"units (bound {om.KERNEL_FACTOR * om.CPU_IDENTITY_UNITS}), |m^2/v/10 - 1| {ratio:.3e} (bound {om.KERNEL_FACTOR * om.CPU_RATIO_REL:.3e})")
        assert ratio <= om.KERNEL_FACTOR * om.CPU_RATIO_REL, (self.n_steps, self.t, ratio)
        assert worst <= om.KERNEL_FACTOR * om.CPU_IDENTITY_UNITS, (self.n_steps, self.t, worst)


def _schedule(d):
    """(b): every transition the product makes, plus the lazy ones.  Nothing is random at run time."""
    mo, o = d.mo, d.opt
    # 1. a local optimisation with a confidence snapshot, closed by the history merge
    d.begin_local(with_confidence=True)
    d.steps(4)
    d.history_merge()
    # 2. an append inside the capacity, steps without a new begin: old rows keep their moments, new rows start from zero
    assert not d.append(N0, N0 + 400)
    assert o.step_count == 4
    d.steps(3)
    # 3. a removal among the trainable rows, steps without a begin: the clean is lazy, step_count restarts
    mask = torch.zeros(o.N, dtype=torch.bool, device=DEV)
    mask[o.n_frozen::7] = True
    d.remove(mask, start=o.n_frozen)
    assert o._stale and o.step_count == 7
    d.steps(3)
    assert o.step_count == 3
    # 4. a fresh local optimisation, then a freeze
    d.begin_local()
    d.steps(3)
    mask = torch.zeros(o.N, dtype=torch.bool, device=DEV)
    mask[o.n_frozen::5] = True
    d.freeze(mask)
    d.steps(2)                                                       # ... and steps without a begin: the lazy clean again
    assert o.step_count == 2
    # 5. a global optimisation with the keyframe-triggered rates (position 0, the rest x 0.1)
    d.begin_global(mo.global_lr_scale(final=False))
    d.steps(4)
    assert d.mode is not None or d.moved_xyz_moments_in_global
    d.end_global()
    assert o._scope == "local" and (d.mode is not None or o._lr_scope is None)
    d.steps(2)                                                       # a local step straight behind the end: fresh moments, the local rates
    assert o.step_count == 2
    # 6. appends beyond the capacity: through append_rows_masked once, through append_rows once
    assert d.append(N0 + 400, N0 + 1200, masked=True)
    d.begin_local()
    d.steps(3)
    assert d.append(N0 + 1200, POOL)
    assert o.step_count == 3
    d.steps(2)                                                       # ... the carried moments go on, in the new arrays
    d.begin_local()
    d.steps(2)
    # 7. a removal that reaches into the frozen prefix
    mask = torch.zeros(o.N, dtype=torch.bool, device=DEV)
    mask[5::9] = True
    nf = o.n_frozen
    d.remove(mask)
    assert o.n_frozen < nf
    # 8. a global optimisation that is never ended: the next begin_local ends it
    d.begin_global(None)
    d.steps(2)
    d.begin_local()
    d.steps(3)
    # 9. one autograd step (which records "all") between two step_slam scopes
    mask = torch.zeros(o.N, dtype=torch.bool, device=DEV)
    mask[o.n_frozen + 1::11] = True
    d.remove(mask, start=o.n_frozen)
    d.steps(1, autograd=True)
    assert o._adam_dirty == "all"
    d.begin_local()
    assert o._adam_dirty is None
    d.steps(3)
    assert d.allocations == 2 and d.n_steps <= 60
    return d


@pytest.mark.parametrize("tail_mode", [0, 1])
def test_state_invariants_hold_after_every_operation_of_the_schedule(tail_mode):
    """(a) + (b): after every begin and every lazy clean all of m / v / ever, the seven arena arrays, the row states and the
    scratch are zero (count_nonzero over the full allocations); after every step nothing is non-zero outside the active
    rows, outside `train`, outside the recorded dirty ranges or on a row whose state is not 1; a row with ever == 0 holds
    the parameters it had when the scope began; frozen rows, the suffix in a global optimisation and xyz under a position
    rate of 0 stay bit for bit; step_count follows the scope, total_steps only rises."""
    d = _schedule(_Driver(tail_mode))
    assert d.total == d.opt.total_steps == d.n_steps
    # the product's own lazy clean ran inside step_slam behind the removal of item 3, the freeze of item 4 and the end of item
    # 5, and inside step() in item 9; the others inside a begin
    assert d.lazy_cleans_in_steps == 4 and d.lazy_cleans > 4, (d.lazy_cleans_in_steps, d.lazy_cleans)


def test_three_kernel_tail_lands_where_the_float64_model_lands():
    """(c), tail_mode 1.  Bound: 4 x CPU_DEVIATION_UNITS, in units of ulp32(|p|) + 2^-23 lr per step taken.  The CPU
    figure - adam1 restated in float32 against AdamModel, 50 steps, parameters re-based never / every step / every 7th
    step - is 19.4 units (tests/optimizer_model.py measure_cpu_figures; most of it is bc2_sqrt: 1 - powf(0.999f, t)
    cancels in float32 at small t).  A stale moment, a wrong t, a leaked learning-rate scope or a skipped row deviates by a
    learning rate: 2^23 units at |p| ~ 0, tens of thousands at |p| ~ 1.  Elements that saw 0 < |g| < 1e-17 in the scope are excluded, counted and bounded at 0.1 %."""
    d = _schedule(_Driver(1, mode="teacher"))
    share = d.n_excluded / max(d.n_stepped, 1)
    nz = [g for g in d.grad_log if g[0]]
    print(f"excluded {d.n_excluded} of {d.n_stepped} stepped elements ({share:.2e}); worst deviation {d.worst['deviation']:.3f} units; "
          f"gradients: zero share {sum(g[1] for g in nz) / max(sum(g[0] for g in nz), 1):.3f}, "
          f"smallest non-zero {min(g[2] for g in nz):.3e}, largest {max(g[3] for g in nz):.3e}")
    margins.record("teacher_forced", deviation_units=d.worst["deviation"], bound_units=om.KERNEL_FACTOR * om.CPU_DEVIATION_UNITS,
                   excluded=d.n_excluded, stepped=d.n_stepped, steps=d.n_steps,
                   grad_zero_share=sum(g[1] for g in nz) / max(sum(g[0] for g in nz), 1),
                   grad_min_nonzero=min(g[2] for g in nz), grad_max=max(g[3] for g in nz))
    assert d.n_stepped > 0 and share <= 1e-3


def test_fused_tail_keeps_the_adam_identities():
    """(d), tail_mode 0.  At an element's first step in a scope m^2 / v = (1 - b1)^2 / (1 - b2) = 10 (bound 4 x the CPU
    figure 1.36e-5, which is the float32 rounding of the two betas); at every step p_new = p_old - lr / (1 - b1^t) m_new /
    (sqrt(v_new) / sqrt(1 - b2^t) + eps) with t counted from the scope's begin and the scope's lr (bound 4 x 56.6 units of
    ulp32(|p|) + 2^-23 lr: the CPU figure of one step recomputed in float64 from the restatement's float32 moments)."""
    d = _schedule(_Driver(0, mode="identity"))
    print(f"worst identity {d.worst['identity']:.3f} units, worst ratio {d.worst['ratio']:.3e}, stepped {d.n_stepped}")
    margins.record("identities", identity_units=d.worst["identity"], identity_bound=om.KERNEL_FACTOR * om.CPU_IDENTITY_UNITS,
                   ratio_rel=d.worst["ratio"], ratio_bound=om.KERNEL_FACTOR * om.CPU_RATIO_REL, stepped=d.n_stepped)
    assert d.n_stepped > 0 and d.n_first > 0


def test_the_mappers_fix_skip_never_hides_a_gaussian_over_the_threshold():
    """(e): Mapping.gaussians_fix returns early while no step ran since it last looked.  Over the 15-frame changing stream of
    tests/test_mapping_cpu.py (releases, a large fix) with the product's own kernels: at every early return what the skipped
    body would have computed is computed - no unstable Gaussian is over the threshold; total_steps rises by one per step /
    step_slam and is never reset by a begin, a re-allocation or an append."""
    from rtg_slam_amd import mapping as mp
    from tests import test_mapping_cpu as tm
    dev = torch.device("cuda", 0)
    args = tm._args()
    m = mp.Mapping(args, dev, capacity=300)
    o = m.opt
    seen = dict(steps=0, skipped=0, looked=0, allocations=0, begins=0)

    def counted(fn):
        def call(*a, **k):
            seen["steps"] += 1
            return fn(*a, **k)
        return call
    o.step_slam, o.step = counted(o.step_slam), counted(o.step)
    alloc, begin, fix = o._allocate, o._begin, m.gaussians_fix

    def _allocate(*a, **k):
        before = o.total_steps
        seen["allocations"] += 1
        alloc(*a, **k)
        assert o.total_steps == before
    o._allocate = _allocate

    def _begin(*a, **k):
        before = o.total_steps
        seen["begins"] += 1
        begin(*a, **k)
        assert o.total_steps == before
    o._begin = _begin

    def gaussians_fix(mask=None):
        if mask is None and o.n_train > 0:
            if o.total_steps == getattr(m, "_fix_seen_steps", None):
                seen["skipped"] += 1
                conf_u = m.aux("confidence", "unstable").reshape(-1)
                assert int((conf_u > args.stable_confidence_thres).sum()) == 0
            else:
                seen["looked"] += 1
        return fix(mask)
    m.gaussians_fix = gaussians_fix
    for fid, (d, c, c2w) in enumerate(tm._changing_stream(15)):
        fr = mp.Frame(tm.CAM, c2w, dev, uid=fid)
        fm = {k: (v.to(dev) if torch.is_tensor(v) else v)
              for k, v in tm._frame_map(d, c, mp.Frame(tm.CAM, c2w, torch.device("cpu")), args).items()}
        m.mapping(fr, fm, fid)
        assert o.total_steps == seen["steps"], fid
        m.time += 1
    print(seen, "fixed", m.stats["fixed"], "rows", o.N, "capacity", o.capacity)
    assert seen["skipped"] > 0 and seen["looked"] > 0 and seen["begins"] > 0 and seen["allocations"] > 0
    assert seen["steps"] > 0 and m.stats["fixed"] > 0
