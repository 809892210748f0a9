"""A plain float64 model of what ShardedMapOptimizer (rtg_slam_amd/map_optim.py) has to compute, for the optimiser-state
tests (tests/test_optimizer_state_cpu.py, tests/test_optimizer_state_gpu.py).  CPU, torch and numpy only.

The reference creates a new torch.optim.Adam for every local or global optimisation (mapper.py:156, :627; betas 0.9 / 0.999,
eps 1e-15).  `AdamModel` restates that per SCOPE: float64 parameters and moments over the rows the scope trains, a step
counter that starts at 0, the learning-rate columns of the scope and the attach snapshot (mapper.py:147-153, 384-401).  It is
TEACHER-FORCED: `step` is handed the float32 gradient rows the product itself produced, so the order in which the
rasterizer summed them - and the sign of a ~0 gradient, which Adam at eps 1e-15 turns into a learning-rate-sized move - is
not part of the comparison.  What is left is the optimiser: which rows are stepped, from which moments, with which `t`
and which learning rate.

A row is stepped by the product's own rule (map_ops.hip map_tail_rows_kernel, map_fused.hip): per block (xyz / SH / raw8),
if it carries gradient now or was stepped earlier in this scope.  The xyz gradient of the attach regulariser is not among
the rows the product leaves behind: the model computes it, 2000 (p - p0) / (3 n_sel), from its own parameters and the
snapshot, for the rows the kernel applies it to; the raw8 part of that term is inside the product's raw8 gradient row.

`adam1_f32` is a numpy float32 restatement of rtg_slam_amd/csrc/adam_common.h `adam1` (same operation order, every
operation rounded on its own - no fused multiply-add).  The tolerances of the GPU tests are derived from the distance
between it and `AdamModel` (`measure_cpu_figures`), never from a run of the code under test."""
from __future__ import annotations

import numpy as np
import torch

B1, B2, EPS = 0.9, 0.999, 1e-15
COLS = 59
BLOCKS = (("xyz", 0, 3), ("shs", 3, 51), ("raw8", 51, 59))
TINY_GRAD = 1e-17            # below it (1 - beta2) g^2 leaves float32's normal range: float64 legitimately disagrees

# Measured by measure_cpu_figures() (tests/test_optimizer_state_cpu.py asserts that a fresh measurement stays at or under
# them).  DEVIATION: largest |float32 restatement - AdamModel| of a parameter, in units of ulp32(|p|) + 2^-23 lr per step
# taken.  IDENTITY: the same unit, for one step recomputed in float64 from the float32 moments the step left.  RATIO:
# largest relative distance of m^2 / v from 10 after an element's first step.  The GPU tests allow 4 x each (the kernel's
# fused multiply-adds round differently from the restatement).
CPU_DEVIATION_UNITS = 19.4
CPU_IDENTITY_UNITS = 56.6
CPU_RATIO_REL = 1.36e-5
KERNEL_FACTOR = 4.0


def ulp32(x):
    """Spacing of float32 at |x| (numpy array in, float64 array out)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def unit(p, lr):
    """The unit the tolerances are counted in: one float32 ulp of the parameter plus one relative float32 rounding of a
    learning-rate-sized move."""
    return ulp32(p) + 2.0 ** -23 * np.asarray(lr, dtype=np.float64)


def adam1_f32(p, g, m, v, lr, step, eps=EPS, b1=B1, b2=B2):
    """adam_common.h adam1 on float32 numpy arrays; returns (p, m, v).  bc1 / bc2_sqrt as the launchers form them
    (1 - powf(beta, step), sqrtf of it) - all in float32, no contraction."""
    f = np.float32
    p, g, m, v, lr = (np.asarray(a, dtype=f) for a in (p, g, m, v, lr))
    b1, b2, eps = f(b1), f(b2), f(eps)
    bc1 = f(1) - f(np.power(b1, f(step), dtype=f))
    bc2s = f(np.sqrt(f(1) - f(np.power(b2, f(step), dtype=f)), dtype=f))
    t1 = (f(1) - b1) * g
    t2 = ((f(1) - b2) * g) * g
    m = (b1 * m).astype(f) + t1
    v = (b2 * v).astype(f) + t2
    denom = (np.sqrt(v, dtype=f) / bc2s).astype(f) + eps
    st = (lr / bc1).astype(f)
    return (p - (st * (m / denom).astype(f)).astype(f)).astype(f), m.astype(f), v.astype(f)


def expected_update(p_old, m_new, v_new, lr, t, eps=EPS, b1=B1, b2=B2):
    """p_old - lr / (1 - b1^t) * m_new / (sqrt(v_new) / sqrt(1 - b2^t) + eps) in float64 (numpy)."""
    p_old, m_new, v_new, lr = (np.asarray(a, dtype=np.float64) for a in (p_old, m_new, v_new, lr))
    return p_old - lr / (1 - b1 ** t) * m_new / (np.sqrt(v_new) / np.sqrt(1 - b2 ** t) + eps)


class AdamModel:
    """The map as float64 rows [N, 59] with a frozen prefix, and the optimiser state of the running scope.

    `lr_col`: float32 [59], the learning-rate columns of a local optimisation; a global optimisation multiplies them by
    its `lr_scale` (in float32, as the product forms them) for its duration.  Every operation that is not a step takes the
    product's current float32 parameters (`p32`) and continues from them ("re-basing"): the model then measures the steps
    of one stretch, and `steps_taken` counts, per element, the steps since."""

    def __init__(self, packed, n_frozen, lr_col, eps=EPS):
        self.p = packed.detach().cpu().double().clone()
        self.n_frozen = int(n_frozen)
        self.lr_base = lr_col.detach().cpu().float().clone()
        self.eps = float(eps)
        self.scope = "local"
        self.lr_scale = None
        self._fresh()

    # ------------------------------------------------------------------ bookkeeping
    @property
    def N(self):
        return int(self.p.shape[0])

    def rows(self):
        """(first, end) of the rows the scope trains: the unstable suffix, or - in a global optimisation - the stable prefix."""
        return (0, self.n_frozen) if self.scope == "global" else (self.n_frozen, self.N)

    @property
    def lr(self):
        """float64 [59]: the learning-rate columns in force."""
        lr = self.lr_base if self.lr_scale is None else self.lr_base * self.lr_scale
        return lr.double()

    def _fresh(self):
        """A new Adam: zero moments, t = 0, no attach snapshot."""
        r0, r1 = self.rows()
        n = r1 - r0
        self.m = torch.zeros(n, COLS, dtype=torch.float64)
        self.v = torch.zeros(n, COLS, dtype=torch.float64)
        self.ever = torch.zeros(n, 3, dtype=torch.bool)            # stepped earlier in this scope: xyz, SH, raw8
        self.step_count = 0
        self.snapshot = None
        self.history = None
        self.tiny = torch.zeros(n, COLS, dtype=torch.bool)         # saw a gradient below TINY_GRAD in this scope
        self.steps_taken = torch.zeros(n, COLS, dtype=torch.int64)
        self.p_begin = self.p[r0:r1].clone()

    def rebase(self, p32):
        """Continue from the product's float32 parameters [N, 59]."""
        assert tuple(p32.shape) == tuple(self.p.shape)
        self.p = p32.detach().cpu().double().clone()
        self.steps_taken.zero_()

    def _snapshot(self, confidence):
        r0, r1 = self.rows()
        p0 = self.p[r0:r1].clone()
        sel = torch.sigmoid(p0[:, 51]) < 0.9                        # opacity_activation(init_stat["opacity"]) < 0.9
        self.snapshot = dict(p=p0, sel=sel, n_sel=max(int(sel.sum()), 1))
        self.p_begin = p0.clone()
        if confidence is not None:
            self.history = confidence.detach().cpu().double().reshape(-1).clone()

    # ------------------------------------------------------------------ the product's transitions
    def begin_local(self, p32=None, confidence=None):
        self.scope, self.lr_scale = "local", None
        if p32 is not None:
            self.p = p32.detach().cpu().double().clone()
        self._fresh()
        self._snapshot(confidence)

    def begin_global(self, lr_scale=None, p32=None):
        assert self.n_frozen > 0
        self.scope = "global"
        self.lr_scale = None if lr_scale is None else lr_scale.detach().cpu().float().clone()
        if p32 is not None:
            self.p = p32.detach().cpu().double().clone()
        self._fresh()
        self._snapshot(None)

    def end_global(self):
        """Back to the local form; the next step starts a new Adam without a snapshot."""
        if self.scope == "local":
            return
        self.scope, self.lr_scale = "local", None
        self._fresh()

    def append(self, packed_new):
        """New trainable rows behind the last one: the old rows keep their moments and `t`, the new ones start from zero; the
        snapshot no longer covers the rows, so the attach term is off until the next begin."""
        assert self.scope == "local"
        k = int(packed_new.shape[0])
        if k == 0:
            return
        self.p = torch.cat([self.p, packed_new.detach().cpu().double()])
        z = lambda t, fill=0: torch.cat([t, torch.full((k,) + tuple(t.shape[1:]), fill, dtype=t.dtype)])
        self.m, self.v, self.ever, self.tiny, self.steps_taken = z(self.m), z(self.v), z(self.ever), z(self.tiny), z(self.steps_taken)
        self.p_begin = torch.cat([self.p_begin, packed_new.detach().cpu().double()])
        self.snapshot = None
        self.history = None

    def _permute(self, index, n_frozen):
        assert self.scope == "local"
        self.p = self.p[index].clone()
        self.n_frozen = int(n_frozen)
        self._fresh()

    def remove(self, mask):
        mask = mask.detach().cpu().bool().reshape(-1)
        self._permute(torch.nonzero(~mask).reshape(-1), self.n_frozen - int(mask[:self.n_frozen].sum()))

    def freeze(self, mask):
        """The trainable rows under `mask` move, in order, behind the frozen prefix."""
        mask = mask.detach().cpu().bool().reshape(-1).clone()
        nf = self.n_frozen
        mask[:nf] = False
        idx = torch.arange(self.N)
        order = torch.cat([idx[:nf], idx[mask], idx[nf:][~mask[nf:]]])
        self._permute(order, nf + int(mask.sum()))

    def history_merge(self, confidence_now, max_weight=0.5):
        """Mapping.history_merge (mapper.py:212-251) through the oracle tests/test_trainable_gpu.py pins the kernel to."""
        from oracle import slam_ops_oracle as so
        assert self.snapshot is not None and self.history is not None
        r0, r1 = self.rows()
        if r1 == r0 or max_weight <= 0:
            return
        b, t = self.p[r0:r1], self.snapshot["p"]
        xyz, shs, raw8 = so.history_merge(b[:, 0:3], b[:, 3:51], b[:, 51:59], t[:, 0:3], t[:, 3:51], t[:, 51:59],
                                          self.history.reshape(-1, 1), confidence_now.detach().cpu().double().reshape(-1, 1),
                                          max_weight)
        self.p[r0:r1] = torch.cat([xyz, shs, raw8], dim=1)

    # ------------------------------------------------------------------ one step
    def live_masks(self, has_grad):
        """(stepped [n, 59], attach-selected [n]) by the product's rule for the rows that carry render gradient now."""
        rg = has_grad.detach().cpu().bool().reshape(-1)
        e_xyz, e_shs, e_raw8 = self.ever[:, 0], self.ever[:, 1], self.ever[:, 2]
        sel = torch.zeros_like(rg)
        if self.snapshot is not None:
            # a row that was never stepped still equals its snapshot: the kernels do not look at it
            sel = self.snapshot["sel"] & (rg | e_raw8 | e_xyz)
        grad = rg | sel
        live = torch.zeros(rg.shape[0], COLS, dtype=torch.bool)
        live[:, 0:3] = (grad | e_xyz)[:, None]
        live[:, 3:51] = (rg | e_shs)[:, None]
        live[:, 51:59] = (grad | e_raw8)[:, None]
        return live, sel

    def step(self, g_xyz, g_shs, g_raw8, has_grad):
        """`g_*`: the product's float32 gradient rows of the scope's rows ([n,3], [n,48] or [n,16,3], [n,8]); `has_grad`
        [n]: the rows the rasterizer's backward reached (row state 1).  Returns the mask [n, 59] of the stepped elements."""
        r0, r1 = self.rows()
        n = r1 - r0
        rg = has_grad.detach().cpu().bool().reshape(-1)
        live, sel = self.live_masks(rg)
        g = torch.zeros(n, COLS, dtype=torch.float64)
        g[:, 0:3] = g_xyz.detach().cpu().double().reshape(n, 3) * rg[:, None]
        g[:, 3:51] = g_shs.detach().cpu().double().reshape(n, 48) * rg[:, None]
        g[:, 51:59] = g_raw8.detach().cpu().double().reshape(n, 8) * (rg | sel)[:, None]     # render + attach terms, as stored
        p = self.p[r0:r1]
        if self.snapshot is not None and bool(sel.any()):
            k3 = 2000.0 / (3.0 * self.snapshot["n_sel"])
            g[:, 0:3] += k3 * (p[:, 0:3] - self.snapshot["p"][:, 0:3]) * sel[:, None]
        self.step_count += 1
        t = self.step_count
        self.tiny |= live & (g != 0) & (g.abs() < TINY_GRAD)
        m = torch.where(live, B1 * self.m + (1 - B1) * g, self.m)
        v = torch.where(live, B2 * self.v + (1 - B2) * g * g, self.v)
        upd = self.lr[None, :] / (1 - B1 ** t) * m / (v.sqrt() / (1 - B2 ** t) ** 0.5 + self.eps)
        self.p[r0:r1] = torch.where(live, p - upd, p)
        self.m, self.v = m, v
        self.ever |= torch.stack([live[:, 0], live[:, 3], live[:, 51]], dim=1)
        self.steps_taken += live.to(torch.int64)
        return live


# ---------------------------------------------------------------------- the CPU reference pair: where the tolerances come from
def synthetic_gradients(n_rows, n_steps, seed, p_zero=0.02, p_row_off=0.4, p_tiny=1e-5):
    """Gradient streams shaped like the schedule's (the rows the three-kernel tail leaves in the arena over
    tests/test_optimizer_state_gpu.py's schedule: about 2 % exact zeros inside rows that carry gradient, non-zero magnitudes
    from 7e-2 down to 1e-19): magnitudes log-uniform over 1e-16 .. 1e-1 with random signs, `p_zero` exact zeros, `p_tiny`
    of the elements below TINY_GRAD (1e-20 .. 1e-17, the excluded kind), and rows that carry gradient in some steps only
    (they stay live once stepped)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_steps):
        mag = 10.0 ** (-16.0 + 15.0 * torch.rand(n_rows, COLS, generator=g, dtype=torch.float64))
        tiny = 10.0 ** (-20.0 + 3.0 * torch.rand(n_rows, COLS, generator=g, dtype=torch.float64))
        mag = torch.where(torch.rand(n_rows, COLS, generator=g) < p_tiny, tiny, mag)
        sign = torch.where(torch.rand(n_rows, COLS, generator=g) < 0.5, -1.0, 1.0).double()
        val = (mag * sign).float()
        val[torch.rand(n_rows, COLS, generator=g) < p_zero] = 0.0
        on = torch.rand(n_rows, generator=g) >= p_row_off
        out.append((val * on[:, None], on))
    return out


def measure_cpu_figures(n_rows=400, n_steps=50, seed=7, lr_col=None, rebase_every=(0, 1, 7)):
    """adam1_f32 (float32, the kernel's operation order) against AdamModel (float64) on synthetic_gradients, with the
    parameters re-based onto the float32 side never, every step and every 7th step.  Returns
    dict(deviation=, identity=, ratio=, tiny_share=): see CPU_DEVIATION_UNITS / CPU_IDENTITY_UNITS / CPU_RATIO_REL."""
    from rtg_slam_amd import map_optim as mo
    lr32 = (mo.default_lr_columns() if lr_col is None else lr_col).float()
    gen = torch.Generator().manual_seed(seed + 1)
    p0 = torch.cat([4.0 * torch.rand(n_rows, 3, generator=gen) - 2.0, 1.5 * torch.randn(n_rows, 3, generator=gen),
                    0.05 * torch.randn(n_rows, 45, generator=gen), torch.full((n_rows, 1), 4.595),
                    -3.0 - 3.0 * torch.rand(n_rows, 3, generator=gen), torch.randn(n_rows, 4, generator=gen)], dim=1).float()
    worst = dict(deviation=0.0, identity=0.0, ratio=0.0)
    n_tiny = n_stepped = 0
    for every in rebase_every:
        model = AdamModel(p0, 0, lr32)
        model.begin_local()
        model.snapshot = None                                     # the attach term is a gradient like any other: not part of this pair
        p, m, v = p0.numpy().copy(), np.zeros((n_rows, COLS), np.float32), np.zeros((n_rows, COLS), np.float32)
        for t, (g, on) in enumerate(synthetic_gradients(n_rows, n_steps, seed), start=1):
            first = ~model.ever.clone()
            live = model.step(g[:, 0:3], g[:, 3:51], g[:, 51:59], on).numpy()
            pn, mn, vn = adam1_f32(p, g.numpy(), m, v, lr32.numpy()[None, :], t)
            want = expected_update(p, mn, vn, lr32.numpy()[None, :].astype(np.float64), t)
            u = unit(pn, lr32.numpy()[None, :])
            ok = live & ~model.tiny.numpy()
            worst["identity"] = max(worst["identity"], float((np.abs(pn.astype(np.float64) - want) / u)[ok].max()))
            p, m, v = np.where(live, pn, p), np.where(live, mn, m), np.where(live, vn, v)
            taken = np.maximum(model.steps_taken.numpy(), 1)
            dev = np.abs(p.astype(np.float64) - model.p.numpy()) / (u * taken)
            worst["deviation"] = max(worst["deviation"], float(dev[ok].max()))
            fresh = live & np.repeat(first.numpy(), [3, 48, 8], axis=1) & (vn >= np.finfo(np.float32).tiny) & ok
            if fresh.any():
                ratio = m.astype(np.float64) ** 2 / np.where(fresh, v, 1).astype(np.float64)
                worst["ratio"] = max(worst["ratio"], float(np.abs(ratio / 10.0 - 1.0)[fresh].max()))
            if every and t % every == 0:
                model.rebase(torch.from_numpy(p))
        n_tiny += int((model.tiny & (model.ever.repeat_interleave(torch.tensor([3, 48, 8]), dim=1))).sum())
        n_stepped += int(model.ever.repeat_interleave(torch.tensor([3, 48, 8]), dim=1).sum())
    worst["tiny_share"] = n_tiny / max(n_stepped, 1)
    return worst
