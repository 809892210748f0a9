"""Replay harness for the map's DEFAULT add path (Mapping.gaussians_add and the end-of-frame bookkeeping with the fused calls of
HipOps: draw_two / rtgs_draw_new_points, bbox_pad, filter_keep, compact_points, knn_stable, new_rows, append_rows_masked,
delete_mask, error_counters) against the TENSOR form of the same path in mapping.py - the form the lifecycle tests pin to the
reference's own Mapping.

ONE product Mapping (the fused side) runs a stream with its whole lifecycle.  Around every gaussians_add and every end-of-frame
bookkeeping the harness
  1. snapshots the state the call starts from (rows, n_frozen, side arrays, time, frame map, frame window) and loads it into a
     second Mapping - the PLAIN side - whose ops have every fused call switched off (PLAIN_OFF) and masked_append False, so each of
     its decisions goes through the tensor branches;
  2. records the pixels the fused side actually drew (a forwarding object in place of HipOps.so) and hands the plain side's
     sample_pixels the same picks pass by pass - after checking them against oracle.slam_ops_oracle.sample_pixels_mask
     (candidates of that mask, distinct, len == min(n, #candidates), with n the PLAIN branch's own n_trans / n_err);
  3. gives the plain side the same inputs for what is not under test: the same rasterizer (its forward is deterministic:
     asserted once per Replay on T_map, depth and both index maps) and the fused side's per-Gaussian error sums (float atomics)
     by memoising accumulate_gaussian_error;
  4. compares: counts, appended rows in the same order (xyz, SH dc, raw opacity, side arrays bit-equal; rotations and raw scales
     within 2e-6; every other column 0), old rows untouched, and after the bookkeeping the surviving rows, counters, confidence,
     ticks and stats.  Decisions (keep, attach, valid, delete, release) must be IDENTICAL; the one excuse is the mean radius of
     the delete mask (float64 in the kernel, float32 in radius.mean()): a row may differ only inside
     |radius - 10 mean64| <= 1e-6 * 10 mean64, and such rows are counted.
FusedTorchOps is a torch double of the fused calls, so that the harness itself (and Mapping's fused branches) run on the CPU."""
from __future__ import annotations

from collections import deque

import numpy as np
import torch

from oracle import slam_ops_oracle as oso
from rtg_slam_amd import map_optim as mo, mapping as mp
from tests import torch_doubles as td
from tests.dist_util import adam_reference
from tests.mapping_doubles import TorchOps

PLAIN_OFF = ("sample_new_points", "draw_two", "filter_keep", "bbox_pad", "compact_points", "new_rows", "knn_stable", "delete_mask",
             "error_counters")
ROT_TOL = SCALE_TOL = 2e-6          # as test_new_gaussian_kernels_equal_the_torch_form for the same arithmetic
BAND = 1e-6                         # relative half-width of the mean-radius band (the rounding of a float32 mean)
STATS = ("deleted_stable", "deleted_unstable", "released")


def radius32(scales):
    """(sum - min) / 2 of the activated scales in float32, summed left to right."""
    s0, s1, s2 = scales[:, 0], scales[:, 1], scales[:, 2]
    return (((s0 + s1) + s2) - torch.minimum(torch.minimum(s0, s1), s2)) / 2


def delete_reference(scales, tick, time_now, window):
    """gaussians_delete's decision with the mean radius in float64 -> (delete bool[n], in_band bool[n], 10 * mean64).  `tick` None:
    the stable cloud's form (no age term).  A row inside the band is one the float32 mean may decide either way."""
    r = radius32(scales.float()).double()
    thr = 10.0 * float(r.mean()) if r.numel() else 0.0
    big = r > thr
    band = (r - thr).abs() <= BAND * thr
    if tick is not None:
        old = (int(time_now) - tick.reshape(-1).long()) > int(window)
        return big | old, band & ~old, thr
    return big, band, thr


class FusedTorchOps(TorchOps):
    """TorchOps + torch doubles of HipOps' fused calls with the kernels' signatures, so that Mapping takes its fused branches on
    the CPU.  Three switches turn a double subtly WRONG (the harness must notice): filter_ratio (the ratio filter_keep uses
    whatever it is handed), new_rows_shift (the row of an existing Gaussian new_rows reads is off by that much) and stale_stable
    (knn_stable keeps its structure when frozen_key changes).  route_stable sends the neighbour query over cat(new, map) through
    knn_stable whatever the size of the stable cloud (Mapping itself waits for 20 000 stable rows)."""

    def __init__(self, args, seed=0):
        super().__init__(args, seed)
        self.draw_log = []
        self.filter_ratio, self.new_rows_shift, self.stale_stable, self.route_stable = None, 0, False, False
        self.opt_of = None
        self._stable_built, self.stable_builds, self.stable_calls = None, 0, 0

    def sample_new_points(self, vertex, normal, color, n, mask, identity_rot):
        sel = oso.sample_pixels_mask(normal, None if mask is None else mask.reshape(normal.shape[:2]).bool())
        idx = torch.nonzero(sel.reshape(-1)).reshape(-1)
        k = min(int(n), int(idx.numel()))
        if k <= 0:
            return None
        pick = idx[torch.randperm(idx.numel(), generator=self.gen)[:k]]
        self.draw_log.append(pick.clone())
        nrm = normal.reshape(-1, 3)[pick]
        nrm = mp.unit_normals(nrm)
        if identity_rot:
            rot = torch.zeros(k, 4)
            rot[:, 0] = 1
        else:
            rot = mp.compute_rot(nrm)
        return vertex.reshape(-1, 3)[pick], nrm, color.reshape(-1, 3)[pick], rot

    def draw_two(self, vertex, normal, color, tmask, emask, counts, n_pixels, uniform_sample_num, transmission_ratio, error_ratio,
                 identity_rot):
        n_t, n_e = counts.tolist()
        ratio = np.float32(n_t) / np.float32(n_pixels)
        n_trans = int(np.float32(transmission_ratio) * ratio * np.float32(uniform_sample_num))
        n_err = int(np.float32(n_e) * np.float32(error_ratio))
        parts = [self.sample_new_points(vertex, normal, color, n, m, identity_rot) for n, m in ((n_trans, tmask), (n_err, emask))]
        return [p for p in parts if p is not None]

    def filter_keep(self, d2, idx, scales, ratio=0.6):
        ratio = ratio if self.filter_ratio is None else self.filter_ratio
        radius = (scales.sum(dim=1) - scales.min(dim=1).values) / 2
        rad = radius[idx.clamp_min(0).long()] * ratio
        return ~((torch.sqrt(d2) < rad) & (idx >= 0)).any(dim=-1)

    def bbox_pad(self, xyz, pad):
        return torch.cat([xyz.min(dim=0)[0] - pad, xyz.max(dim=0)[0] + pad])

    def compact_points(self, keep, xyz, color, opacity_raw, rots):
        keep = keep.bool()
        return xyz[keep], color[keep], opacity_raw[keep], rots[keep], int(keep.sum())

    def new_rows(self, xyz, color, opacity_raw, rots, d2, idx, exist_scales, min_radius, max_radius, scale_factor, xyz_factor):
        n = xyz.shape[0]
        radius = (exist_scales.sum(dim=1) - exist_scales.min(dim=1).values) / 2 if exist_scales.shape[0] else exist_scales.new_zeros(0)
        total_radius = torch.cat([torch.full((n,), 1e-6), radius])
        j = idx.clamp_min(0).long()
        if self.new_rows_shift:
            j = torch.where(j >= n, (j + self.new_rows_shift).clamp(n, total_radius.shape[0] - 1), j)
        dist = torch.sqrt(d2) - 3 * total_radius[j]
        dist = torch.where(idx >= 0, dist, torch.full_like(dist, 1e30))
        invalid = (dist < 0).any(dim=-1)
        scales = torch.sqrt((dist ** 2).sum(dim=-1) / 3).clamp(min_radius, max_radius)
        rows = torch.zeros(n, mo.COLS)
        rows[:, 0:3] = xyz
        rows[:, 3:6] = mp.RGB2SH(color)
        rows[:, 51:52] = opacity_raw
        rows[:, 52:55] = torch.log(scale_factor * scales[:, None] * torch.tensor(xyz_factor, dtype=torch.float32)[None, :])
        rows[:, 55:59] = rots
        return rows, (~invalid).to(torch.uint8)

    def knn_stable(self, opt, all_xyz, nf, query, box):
        key = opt.frozen_key
        self.stable_calls += 1
        if self._stable_built is None or (self._stable_built[0] != key and not self.stale_stable):
            self._stable_built = (key, all_xyz[:nf].clone())
            self.stable_builds += 1
        return oso.knn_query(torch.cat([query, self._stable_built[1], all_xyz[nf:]]), query, 0, box)

    def knn_query(self, ref, query, self_offset=-1, ref_box=None):
        if self.route_stable and self_offset == 0 and self.opt_of is not None:
            opt, nq = self.opt_of(), query.shape[0]
            if opt.n_frozen > 0 and ref.shape[0] == nq + opt.N:
                return self.knn_stable(opt, ref[nq:], opt.n_frozen, query, ref_box)
        return super().knn_query(ref, query, self_offset, ref_box)

    def delete_mask(self, scales, add_tick, time_now, window, sync=True):
        r = radius32(scales)
        thr = (r.double().sum() / max(int(r.numel()), 1)).float() * 10          # the kernel's float64 mean, rounded once
        d = r > thr
        if add_tick is not None:
            d = d | ((int(time_now) - add_tick.reshape(-1)) > int(window))
        count = d.sum().to(torch.int32).reshape(1)
        return d.to(torch.uint8), (int(count.item()) if sync else count)

    def error_counters(self, g_color, g_depth, nf, color_strike_thr, depth_strike_thr, depth_counter, color_counter, limit=10,
                       sync=True):
        depth_counter[:nf, 0] += (g_depth[:nf] > depth_strike_thr).to(depth_counter.dtype)
        color_counter[:nf, 0] += (g_color[:nf] > color_strike_thr).to(color_counter.dtype)
        ddel = depth_counter[:nf, 0] >= limit
        crel = (color_counter[:nf, 0] >= limit) & ~ddel
        counts = torch.stack([ddel.sum(), crel.sum()]).to(torch.int32)
        return ddel.to(torch.uint8), crel.to(torch.uint8), (counts if not sync else tuple(counts.tolist()))


def make_plain(ops):
    """Switch every fused call of `ops` off ON THE INSTANCE: Mapping then takes its tensor branches."""
    for name in PLAIN_OFF:
        setattr(ops, name, None)
    return ops


def _make_opt(ops, packed, lr_col, n_frozen, capacity):
    kw = dict(adam_fn=adam_reference, activate_fn=td.activate8) if isinstance(ops, TorchOps) else {}
    return mo.ShardedMapOptimizer(packed, lr_col=lr_col, n_frozen=n_frozen, capacity=capacity, **kw)


class _SoTap:
    """Stands where HipOps.so stands and forwards everything; the two calls that draw also leave the pixels they drew."""

    def __init__(self, so):
        self._so, self.events = so, []

    def __getattr__(self, name):
        return getattr(self._so, name)

    def draw_new_points(self, passes, vertex_map, normal_map, color_map, identity_rot, want_pick=False):
        out = self._so.draw_new_points(passes, vertex_map, normal_map, color_map, identity_rot, want_pick=True)
        ks = [int(p[2]) for p in passes if int(p[2]) > 0]
        self.events.append(("draw", [t.clone() for t in out[4].long().cpu().split(ks)]))
        return out if want_pick else out[:4]

    def gather_new_points(self, pick, *a):
        self.events.append(("gather", [pick.long().cpu().clone()]))
        return self._so.gather_new_points(pick, *a)


def _match_pixels(part, vertex, color):
    """The pixels of a pass that went through neither call (the k == 3 detour gathers with tensor indexing): the ONE pixel whose
    vertex and colour equal the row, bit for bit."""
    v, c = vertex.reshape(-1, 3), color.reshape(-1, 3)
    out = []
    for i in range(part[0].shape[0]):
        hit = torch.nonzero((v == part[0][i]).all(dim=1) & (c == part[2][i]).all(dim=1)).reshape(-1)
        assert hit.numel() == 1, ("a drawn row matches %d pixels of the frame" % hit.numel())
        out.append(int(hit[0]))
    return torch.tensor(out, dtype=torch.long)


def _passes_of(parts, events, vertex, color):
    passes = []
    for part in parts:
        n = int(part[0].shape[0])
        if events and events[0][0] == "draw":
            got = events.pop(0)[1]
        elif n == 3:
            got = [_match_pixels(part, vertex, color)]
        else:
            assert events and events[0][0] == "gather", "a sampling pass reached neither draw_new_points nor gather_new_points"
            got = events.pop(0)[1]
        assert sum(int(g.numel()) for g in got) == n, (n, [int(g.numel()) for g in got])
        passes += got
    assert not events, events
    return passes


def tap_draws(ops, log):
    """Every sampling pass of `ops` (a HipOps or a FusedTorchOps) appends the flat pixel indices it drew to `log`."""
    if isinstance(ops, FusedTorchOps):
        ops.draw_log = log
        return
    tap = _SoTap(ops.so)
    ops.so = tap
    two, one = ops.draw_two, ops.sample_new_points

    def draw_two(vertex, normal, color, *a):
        tap.events.clear()
        parts = two(vertex, normal, color, *a)
        log.extend(_passes_of(parts, tap.events, vertex, color))
        return parts

    def sample_new_points(vertex, normal, color, *a):
        tap.events.clear()
        part = one(vertex, normal, color, *a)
        if part is not None:
            log.extend(_passes_of([part], tap.events, vertex, color))
        return part
    ops.draw_two, ops.sample_new_points = draw_two, sample_new_points


def frame_maps(device):
    """tests.test_mapping_cpu._frame_map for any camera (the oracle's preprocessing, on the CPU), moved to `device`."""
    def fn(d, c, c2w, cam, args):
        fr = mp.Frame(cam, c2w, torch.device("cpu"))
        fm = oso.frame_preprocess(d.reshape(cam.H, cam.W, 1), fr.K, args.min_depth, 8.0, False, args.invalid_confidence_thresh)
        fm["color_map"] = c.permute(1, 2, 0).contiguous()
        fm["vertex_map_w"] = fm["vertex_map_c"] @ fr.get_c2w[:3, :3].T + fr.get_c2w[:3, 3]
        fm["normal_map_w"] = fm["normal_map_c"] @ fr.get_c2w[:3, :3].T
        return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in fm.items()}
    return fn


def assert_tolerances(seen):
    """The two toleranced comparisons of a replay run with defer_tolerances: printed, then asserted."""
    print(f"largest difference over {seen['rows']} appended rows of {seen['adds']} frames: rotations {seen['rot_max']:.3e} "
          f"(bound {ROT_TOL}; {seen['rot_rows_over']} rows over it), raw scales {seen['scale_max']:.3e} (bound {SCALE_TOL})")
    assert seen["rot_max"] <= ROT_TOL, ("rotations", seen["rot_max"])
    assert seen["scale_max"] <= SCALE_TOL, ("raw scales", seen["scale_max"])


class Replay:
    def __init__(self, fused: mp.Mapping, plain_ops, bookkeeping=True, defer_tolerances=False):
        """defer_tolerances: the two toleranced comparisons (rotations, raw scales) only record their largest difference, for
        assert_tolerances(seen) after the run - every exact comparison of every frame is then made whatever they find."""
        self.defer = bool(defer_tolerances)
        self.f, self.dev = fused, fused.device
        make_plain(plain_ops)
        plain_ops.sample_pixels = self._replay_pixels
        plain_ops.accumulate_gaussian_error = self._memo_error
        self.p = mp.Mapping(fused.args, fused.device, ops=plain_ops, capacity=8)
        self.p.masked_append = False
        self.passes, self.memo, self.masks, self.pending = [], None, {}, None
        self.cap_f, self.cap_p = {}, {}
        self.render_checked = False
        self.seen = dict(frames=0, adds=0, rows=0, rows_bookkeeping=0, books=0, filter_drop=0, attach=0, release=0, del_stable=0,
                         del_unstable=0, excused=0, k3=0, invalid=0, act_max_diff=0.0, rot_max=0.0, scale_max=0.0, cand_rot_max=0.0, rot_rows_over=0,
                         pass_sizes=[])
        tap_draws(fused.ops, self.passes)
        self._wrap_ops(fused.ops)
        self._capture(self.f, self.cap_f)
        self._capture(self.p, self.cap_p)
        self._orig_add = fused.gaussians_add
        fused.gaussians_add = self._add
        if bookkeeping:
            one, remove, delete = fused._error_remove_and_delete, fused.error_gaussians_remove, fused.gaussians_delete

            def error_remove_and_delete():
                self._book_begin()
                one()
                self._book_end()

            def error_gaussians_remove():
                self._book_begin()
                remove()

            def gaussians_delete(unstable=True):
                delete(unstable)
                if unstable and self.pending is not None:
                    self._book_end()
            fused._error_remove_and_delete, fused.error_gaussians_remove, fused.gaussians_delete = \
                error_remove_and_delete, error_gaussians_remove, gaussians_delete

    # ------------------------------------------------------------------ taps
    def _wrap_ops(self, ops):
        acc = ops.accumulate_gaussian_error

        def accumulate(H, W, P, *a):
            out = acc(H, W, P, *a)
            self.memo = (int(P), tuple(t.clone() for t in out))
            return out
        ops.accumulate_gaussian_error = accumulate
        if getattr(ops, "delete_mask", None) is not None:
            dmask = ops.delete_mask

            def delete_mask(*a, **kw):
                out = dmask(*a, **kw)
                self.masks["dm"] = out[0].bool().clone()
                return out
            ops.delete_mask = delete_mask
        if getattr(ops, "error_counters", None) is not None:
            ecnt = ops.error_counters

            def error_counters(*a, **kw):
                out = ecnt(*a, **kw)
                self.masks["ddel"], self.masks["crel"] = out[0].bool().clone(), out[1].bool().clone()
                return out
            ops.error_counters = error_counters

    @staticmethod
    def _capture(m, cap):
        filt, to_opt = m.temp_points_filter, m.temp_to_optimize

        def temp_points_filter(temp, topk=3):
            keep = filt(temp, topk)
            cap.update(xyz=temp["xyz"], color=temp["color"], rots=temp["rots"], normal=temp["normal"], keep=keep.bool().clone())
            return keep

        def temp_to_optimize(temp, keep):
            cap["opacity"] = temp["opacity_raw"].reshape(-1).clone()
            return to_opt(temp, keep)
        m.temp_points_filter, m.temp_to_optimize = temp_points_filter, temp_to_optimize

    def _memo_error(self, H, W, P, *a):
        assert self.memo is not None and self.memo[0] == int(P), "the plain side accumulates errors the fused side did not"
        return self.memo[1]

    def _replay_pixels(self, vertex, normal, color, n, mask):
        H, W = normal.shape[:2]
        sel = oso.sample_pixels_mask(normal.cpu(), None if mask is None else mask.cpu().reshape(H, W).bool())
        cand = torch.nonzero(sel.reshape(-1)).reshape(-1)
        want = min(int(n), int(cand.numel()))
        if want == 0:
            e = vertex.new_zeros(0, 3)
            return e, e.clone(), e.clone()
        assert self.passes, f"the plain side draws {want} pixels in a pass the fused side did not draw"
        pick = self.passes.pop(0)
        assert int(pick.numel()) == want, f"fused pass of {int(pick.numel())} pixels, min(n, candidates) = min({int(n)}, {int(cand.numel())})"
        assert bool(torch.isin(pick, cand).all()), "a drawn pixel is no candidate of its mask"
        assert int(pick.unique().numel()) == want, "a pass drew a pixel twice"
        pick = pick.to(vertex.device)
        return vertex.reshape(-1, 3)[pick], normal.reshape(-1, 3)[pick], color.reshape(-1, 3)[pick]

    # ------------------------------------------------------------------ snapshot
    def _snapshot(self):
        o = self.f.opt
        return dict(params=o.params.clone(), N=o.N, nf=o.n_frozen, cap=max(o.capacity, o.N, 1), time=self.f.time,
                    aux={k: o.aux[k][:o.N].clone() for k in o._aux_spec})

    def _load_plain(self, s):
        f, p = self.f, self.p
        opt = _make_opt(p.ops, s["params"], p.lr_col, s["nf"], s["cap"])
        for name, (width, dtype, fill) in f.opt._aux_spec.items():
            opt.add_aux(name, width, dtype, fill)
            opt.aux[name][:s["N"]] = s["aux"][name]
        opt.add_aux("rid", 1, torch.int32, -1)                   # which snapshot row a surviving row was (plain side only)
        opt.aux["rid"][:s["N"], 0] = torch.arange(s["N"], dtype=torch.int32, device=self.dev)
        p.opt, p.time, p.frame_map, p._render_cache = opt, s["time"], f.frame_map, None
        p.processed_frames = deque(f.processed_frames, maxlen=f.processed_frames.maxlen)
        p.processed_map = deque(f.processed_map, maxlen=f.processed_map.maxlen)
        p.stats = {k: 0 for k in f.stats if k != "last_add"}
        if s["N"]:
            d = (f.opt.gaussian_data("all")["scales"] - opt.gaussian_data("all")["scales"]).abs().max()
            self.seen["act_max_diff"] = max(self.seen["act_max_diff"], float(d))

    def _check_render(self, frame):
        a = self.f.ops.render(frame, self.f.opt.gaussian_data("all"))
        b = self.p.ops.render(frame, self.p.opt.gaussian_data("all"))
        for k in ("T_map", "depth", "color_index_map", "depth_index_map"):
            assert torch.equal(a[k], b[k]), f"two renders of the same rows differ in {k}"
        self.render_checked = True

    # ------------------------------------------------------------------ gaussians_add
    def _add(self, frame):
        f, p = self.f, self.p
        s = self._snapshot()
        self._load_plain(s)
        if not self.render_checked and s["N"] > 0:
            self._check_render(frame)
        self.passes.clear()
        self.cap_f.clear()
        self.cap_p.clear()
        f.stats.pop("last_add", None)
        v0 = f.opt.version
        self._orig_add(frame)
        sizes = [int(t.numel()) for t in self.passes]
        self.last_picks = torch.cat(self.passes) if self.passes else None
        pv0 = p.opt.version
        p.gaussians_add(frame)
        assert not self.passes, f"the fused side drew passes of {sizes}; the plain side left {len(self.passes)} of them undrawn"
        self._compare_add(s, v0, pv0, sizes)

    def _compare_add(self, s, v0, pv0, sizes):
        f, p, cf, cp, seen = self.f, self.p, self.cap_f, self.cap_p, self.seen
        t = s["time"]
        assert ("keep" in cf) == ("keep" in cp), (t, "one side drew candidates, the other none")
        if "keep" in cf:
            assert torch.equal(cf["xyz"], cp["xyz"]) and torch.equal(cf["color"], cp["color"]), (t, "candidates differ")
            seen["cand_rot_max"] = max(seen["cand_rot_max"], float((cf["rots"] - cp["rots"]).abs().max()))    # dropped ones included
            bad = torch.nonzero(cf["keep"] != cp["keep"]).reshape(-1)
            assert bad.numel() == 0, (t, "filter decision differs on candidates", bad.tolist()[:8], "fused keeps", cf["keep"][bad].tolist()[:8])
            if "opacity" in cf or "opacity" in cp:
                bad = torch.nonzero(cf["opacity"] != cp["opacity"]).reshape(-1)
                assert bad.numel() == 0, (t, "attach decision differs on candidates", bad.tolist()[:8], "fused", cf["opacity"][bad].tolist()[:8])
                seen["attach"] += int(bool((cf["opacity"] < 0).any()))
            seen["filter_drop"] += int(not bool(cf["keep"].all()))
        la_f, la_p = f.stats.get("last_add"), p.stats.get("last_add")
        assert la_f == la_p, (t, "(candidates, kept by the filter, accepted): fused", la_f, "plain", la_p)
        N0, N = s["N"], f.opt.N
        assert p.opt.N == N and f.opt.n_frozen == p.opt.n_frozen == s["nf"], (t, N, p.opt.N)
        moved = N > N0
        assert (f.opt.version != v0) == moved and (p.opt.version != pv0) == moved, (t, "version")
        Pf, Pp = f.opt.params, p.opt.params
        for side, P, o in (("fused", Pf, f.opt), ("plain", Pp, p.opt)):
            assert torch.equal(P[:N0], s["params"]), (t, side, "an existing row changed in the add")
            for k, v in s["aux"].items():
                assert torch.equal(o.aux[k][:N0], v), (t, side, k, "an existing row's side array changed in the add")
        if moved:
            a, b = Pf[N0:], Pp[N0:]
            for name, c0, c1 in (("xyz", 0, 3), ("SH dc", 3, 6), ("raw opacity", 51, 52)):
                assert torch.equal(a[:, c0:c1], b[:, c0:c1]), (t, name, float((a[:, c0:c1] - b[:, c0:c1]).abs().max()),
                                                               int((a[:, c0:c1] != b[:, c0:c1]).any(dim=1).sum()), "rows of", N - N0)
            assert float(a[:, 6:51].abs().max()) == 0.0 and float(b[:, 6:51].abs().max()) == 0.0, (t, "SH rest")
            d_scale, d_rot = float((a[:, 52:55] - b[:, 52:55]).abs().max()), float((a[:, 55:59] - b[:, 55:59]).abs().max())
            seen["scale_max"], seen["rot_max"] = max(seen["scale_max"], d_scale), max(seen["rot_max"], d_rot)
            seen["rot_rows_over"] += int(((a[:, 55:59] - b[:, 55:59]).abs().max(dim=1).values > ROT_TOL).sum())
            assert self.defer or d_scale <= SCALE_TOL, (t, "raw scales", d_scale)
            assert self.defer or d_rot <= ROT_TOL, (t, "rotations", d_rot)
            for k in s["aux"]:
                assert torch.equal(f.opt.aux[k][N0:N], p.opt.aux[k][N0:N]), (t, k)
            assert bool((f.opt.aux["add_tick"][N0:N] == t).all())
            seen["adds"] += 1
            seen["rows"] += N - N0
            seen["invalid"] += int(la_f[1] > la_f[2])
        seen["k3"] += sum(1 for k in sizes if k == 3)
        seen["pass_sizes"].append(sizes)

    # ------------------------------------------------------------------ end-of-frame bookkeeping
    def _book_begin(self):
        s = self._snapshot()
        self._load_plain(s)
        s["stats"] = {k: self.f.stats[k] for k in STATS}
        u = self.p.opt.gaussian_data("unstable")["scales"]
        s["ref"] = delete_reference(u.clone(), s["aux"]["add_tick"][s["nf"]:], s["time"], self.f.args.unstable_time_window) \
            if s["N"] > s["nf"] else None
        self.masks.clear()
        self.memo = None
        self.pending = s

    def _book_end(self):
        f, p, s, seen = self.f, self.p, self.pending, self.seen
        self.pending = None
        p.error_gaussians_remove()
        p.gaussians_delete()
        t, N0, nf0, dev = s["time"], s["N"], s["nf"], self.dev
        zeros = lambda n: torch.zeros(n, dtype=torch.bool, device=dev)
        ddel, dm = self.masks.get("ddel", zeros(nf0)), self.masks.get("dm", zeros(N0 - nf0))
        ids_f = torch.nonzero(~torch.cat([ddel, dm])).reshape(-1)
        assert int(ids_f.numel()) == f.opt.N and f.opt.n_frozen == nf0 - int(ddel.sum()), (t, "fused: rows left do not match its masks")
        ids_p = p.opt.aux["rid"][:p.opt.N, 0].long()
        del_p = torch.ones(N0, dtype=torch.bool, device=dev)
        del_p[ids_p] = False
        bad = torch.nonzero(del_p[:nf0] != ddel).reshape(-1)
        assert bad.numel() == 0, (t, "stable delete decision differs on rows", bad.tolist()[:8])
        excused = 0
        if s["ref"] is not None:
            want, band, thr = s["ref"]
            for side, got in (("fused", dm), ("plain", del_p[nf0:])):
                bad = torch.nonzero((got != want) & ~band).reshape(-1)
                assert bad.numel() == 0, (t, side, "unstable delete decision against the float64 mean: rows", bad.tolist()[:8], "10 x mean64", thr)
            excused = int((dm != del_p[nf0:]).sum())                # all inside the band, by the two assertions above
        seen["excused"] += excused
        if excused == 0:
            assert torch.equal(ids_f, ids_p), (t, "surviving rows")
            assert p.opt.N == f.opt.N and p.opt.n_frozen == f.opt.n_frozen
        in_f, in_p = torch.isin(ids_f, ids_p), torch.isin(ids_p, ids_f)
        Pf, Pp = f.opt.params[in_f], p.opt.params[in_p]
        assert torch.equal(Pf, Pp), (t, "surviving rows' parameters")
        assert torch.equal(Pf, s["params"][ids_f[in_f]]), (t, "a surviving row changed")
        for k in s["aux"]:
            assert torch.equal(f.opt.aux[k][:f.opt.N][in_f], p.opt.aux[k][:p.opt.N][in_p]), (t, k)
        d = {k: f.stats[k] - s["stats"][k] for k in STATS}
        for k in STATS:
            if k != "deleted_unstable" or excused == 0:
                assert d[k] == p.stats[k], (t, k, d[k], p.stats[k])
        seen["books"] += 1
        seen["rows_bookkeeping"] += N0
        seen["release"] += int(d["released"] > 0)
        seen["del_stable"] += int(d["deleted_stable"] > 0)
        seen["del_unstable"] += int(d["deleted_unstable"] > 0)

    # ------------------------------------------------------------------ driving
    def run(self, stream, cam, frame_map_fn, after_frame=None):
        m = self.f
        for fid, (d, c, c2w) in enumerate(stream):
            fr = mp.Frame(cam, c2w, self.dev, uid=fid)
            m.mapping(fr, frame_map_fn(d, c, c2w, cam, m.args), fid)
            m.get_render_output(fr)
            m.time += 1
            self.seen["frames"] += 1
            if after_frame is not None:
                after_frame(fid)
        return self.seen
