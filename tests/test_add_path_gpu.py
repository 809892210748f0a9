"""The product's default add path - HipOps' fused calls, as Mapping.gaussians_add and the end-of-frame bookkeeping chain them -
against the tensor form of the same path (tests/add_path_replay.py) on the states of real lifecycles, and the single-workgroup
kernels of that path at and past the sizes their comments assume."""
import functools

import numpy as np
import pytest
import torch

from oracle import slam_ops_oracle as oso
from rtg_slam_amd import map_optim as mo, mapping as mp, synth
from tests import add_path_replay as rp, margins, test_mapping_cpu as tm
from tests.test_add_path_cpu import check_not_vacuous

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
AUX = (("confidence", torch.float32, 0.0), ("add_tick", torch.int32, 0), ("depth_error_counter", torch.int32, 0),
       ("color_error_counter", torch.int32, 0))


@functools.lru_cache(maxsize=None)
def _lifecycle(n_frames, changing, ratios=()):
    """One replayed lifecycle per stream and argument set, shared by the tests that read it.  The two toleranced comparisons are
    deferred to test_rotations_and_raw_scales_of_the_appended_rows, so that every exact comparison of every frame is made."""
    args = tm._args(**dict(ratios))
    m = mp.Mapping(args, DEV, capacity=600)                         # the default ops: HipOps
    assert isinstance(m.ops, mp.HipOps) and m.masked_append and m.ops.kernel_draw
    r = rp.Replay(m, mp.HipOps(args, DEV), defer_tolerances=True)
    seen = r.run((tm._changing_stream if changing else tm._stream)(n_frames), tm.CAM, rp.frame_maps(DEV))
    print(seen)
    assert r.render_checked
    margins.record("add_path", frames=seen["frames"], rows_added=seen["rows"], rows_bookkeeping=seen["rows_bookkeeping"],
                   rows_excused_mean_band=seen["excused"], activation_max_diff=seen["act_max_diff"], passes_of_three=seen["k3"],
                   rotations_max_diff=seen["rot_max"], raw_scales_max_diff=seen["scale_max"])
    return seen


# ---------------------------------------------------------------------------------------------------------------- a. lifecycle
@pytest.mark.parametrize("n_frames,changing", [(7, False), (15, True)])
def test_the_default_add_path_equals_its_tensor_form_through_a_lifecycle(n_frames, changing):
    """Every gaussians_add and every end-of-frame bookkeeping of the streams the lifecycle tests pin to the reference's own
    Mapping: identical decisions, appended rows in the same order, the same survivors, counters, confidence and ticks."""
    check_not_vacuous(_lifecycle(n_frames, changing), n_frames, changing)


THREE = [(("error_sample_ratio", 0.005),), (("transmission_sample_ratio", 0.019),)]


@pytest.mark.parametrize("ratios", THREE)
def test_a_pass_of_exactly_three_points_inside_the_lifecycle(ratios):
    """Ratios under which (on the CPU doubles) five or six of the seven frames draw exactly 3 points in the error pass / in the
    transmission pass: draw_two's k == 3 detour (randperm + compute_rot's batch-of-three rule) with either pass order."""
    seen = _lifecycle(7, False, ratios)
    assert seen["k3"] >= 1 and seen["adds"] >= 6, seen
    first = ratios[0][0] == "transmission_sample_ratio"
    assert any(len(s) == 2 and s[0 if first else 1] == 3 and s[1 if first else 0] > 3 for s in seen["pass_sizes"]), seen["pass_sizes"]


# ---------------------------------------------------------------------------------------------------------------- b. draw sizes
def _draw_frame():
    gen = torch.Generator().manual_seed(31)
    H, W = 60, 80
    vertex = torch.randn(H, W, 3, generator=gen)
    normal = torch.nn.functional.normalize(torch.randn(H, W, 3, generator=gen), dim=-1) * 0.97
    normal.reshape(-1, 3)[::41] = 0                                  # pixels without a normal: in a mask, but no candidates
    color = torch.rand(H, W, 3, generator=gen)
    return H, W, vertex.to(DEV), normal.to(DEV), color.to(DEV)


def _range_mask(H, W, lo, hi):
    m = torch.zeros(H * W, dtype=torch.uint8)
    m[lo:hi] = 1
    return m.reshape(H, W)


# (pixels of the transmission mask, of the error mask, uniform_sample_num, transmission ratio, error ratio) -> the (k_t, k_e) wanted
DRAW_CASES = {
    "0,0": ((0, 0), (0, 0), 4800, 1.0, 0.05, (0, 0)),
    "0,k": ((0, 0), (1000, 1400), 4800, 1.0, 0.05, (0, 20)),
    "k,0": ((100, 600), (2000, 2010), 4800, 0.5, 0.05, (250, 0)),
    "3,k": ((42, 45), (1000, 1400), 9600, 1.0, 0.05, (3, 20)),       # three candidates cap the first pass
    "k,3": ((100, 600), (2000, 2070), 4800, 0.5, 0.05, (250, 3)),    # int(70 * 0.05) = 3
    "1,1": ((42, 43), (2000, 2030), 9600, 1.0, 0.05, (1, 1)),
    "caps": ((100, 300), (2000, 2100), 48000, 1.0, 2.0, None),        # both passes take every candidate of their mask
}


@pytest.mark.parametrize("case", list(DRAW_CASES))
@pytest.mark.parametrize("identity_rot", [False, True])
def test_draw_two_sizes_layout_and_rows(case, identity_rot):
    """HipOps.draw_two alone: the sizes follow min(n, candidates) with n from the float32 arithmetic of the tensor branch, pass 1
    occupies rows [0, k_t), every pick is a distinct candidate of its pass's mask, and the rows are rtgs_gather_new_points of
    those picks (a pass of 3: the tensor form with compute_rot's rule)."""
    from rtg_slam_amd import slam_ops
    H, W, vertex, normal, color = _draw_frame()
    (t0, t1), (e0, e1), usn, tr, er, want = DRAW_CASES[case]
    tmask, emask = _range_mask(H, W, t0, t1).to(DEV), _range_mask(H, W, e0, e1).to(DEV)
    counts = torch.tensor([t1 - t0, e1 - e0], dtype=torch.int32, device=DEV)
    cands = [torch.nonzero(oso.sample_pixels_mask(normal.cpu(), m.cpu().bool()).reshape(-1)).reshape(-1) for m in (tmask, emask)]
    n_trans = int(np.float32(tr) * (np.float32(t1 - t0) / np.float32(H * W)) * np.float32(usn))        # mapping.py's tensor branch
    n_err = int(np.float32(e1 - e0) * np.float32(er))
    ks = (min(n_trans, int(cands[0].numel())), min(n_err, int(cands[1].numel())))
    if want is None:
        assert ks == (int(cands[0].numel()), int(cands[1].numel())) and ks[0] < t1 - t0 and ks[1] < e1 - e0, ks
    else:
        assert ks == want, (ks, want)
    args = tm._args(seed=7)
    m = mp.Mapping(args, DEV, capacity=8)
    log = []
    rp.tap_draws(m.ops, log)
    parts = m.ops.draw_two(vertex, normal, color, tmask, emask, counts, H * W, usn, tr, er, identity_rot)
    new = m._new_points(parts)
    if ks == (0, 0):
        assert new is None and not log
        return
    assert [int(p.numel()) for p in log] == [k for k in ks if k > 0]
    assert new["xyz"].shape == (sum(ks), 3) and new["rots"].shape == (sum(ks), 4) and new["opacity_raw"].shape == (sum(ks), 1)
    off = 0
    for k, cand in zip(ks, cands):
        if k == 0:
            continue
        pick = log.pop(0)
        assert bool(torch.isin(pick, cand).all()) and int(pick.unique().numel()) == k
        pick = pick.to(DEV)
        rows = {key: new[key][off:off + k] for key in ("xyz", "normal", "color", "rots")}
        if k == 3:
            nrm = normal.reshape(-1, 3)[pick]
            nrm = mp.unit_normals(nrm)
            rot = torch.tensor([1.0, 0, 0, 0], device=DEV).repeat(3, 1) if identity_rot else mp.compute_rot(nrm)
            ref = (vertex.reshape(-1, 3)[pick], nrm, color.reshape(-1, 3)[pick], rot)
        else:
            ref = slam_ops.gather_new_points(pick, vertex, normal, color, identity_rot)
        for key, want_rows in zip(("xyz", "normal", "color", "rots"), ref):
            assert torch.equal(rows[key], want_rows), (case, key)
        off += k
    assert float(new["opacity_raw"].min()) == float(new["opacity_raw"].max()) == np.float32(mp.inverse_sigmoid(args.init_opacity))


# ---------------------------------------------------------------------------------------------------------------- c. stable prefix
BIG = synth.CameraSpec(120, 160, 100.0, 100.0, 79.5, 59.5)
N_STABLE = 21000


def _seeded(n_unstable, capacity, args):
    """A Mapping at time 5 whose map is a surface cloud of the box room: N_STABLE frozen rows, n_unstable trainable ones (discs
    shrunk to 15 % so that the room still has gaps and new points are not all inside three radii of a neighbour)."""
    n = N_STABLE + n_unstable
    g = synth.surface_gaussians(n, BIG, seed=5)
    g["scales"] = g["scales"] * 0.15
    packed = mo.pack_from_activated({k: v.to(DEV) for k, v in g.items()})
    m = mp.Mapping(args, DEV, capacity=8)
    opt = mo.ShardedMapOptimizer(packed, lr_col=m.lr_col, n_frozen=N_STABLE, capacity=capacity)
    gen = torch.Generator().manual_seed(3)
    for name, dtype, fill in AUX:
        opt.add_aux(name, 1, dtype, fill)
    opt.aux["confidence"][:N_STABLE, 0] = args.stable_confidence_thres
    opt.aux["confidence"][N_STABLE:n, 0] = torch.rand(n_unstable, generator=gen).to(DEV)
    opt.aux["add_tick"][:n, 0] = torch.randint(2, 6, (n,), generator=gen, dtype=torch.int32).to(DEV)
    opt.aux["depth_error_counter"][:n, 0] = torch.randint(0, 5, (n,), generator=gen, dtype=torch.int32).to(DEV)
    opt.aux["color_error_counter"][:n, 0] = torch.randint(0, 5, (n,), generator=gen, dtype=torch.int32).to(DEV)
    m.opt, m.time = opt, 5
    return m


def _big_args(uniform_sample_num=1500):
    return tm._args(uniform_sample_num=uniform_sample_num, seed=5)


def _big_frames(n):
    out = []
    for p in synth.trajectory(n, seed=9):
        d = synth.box_room_depth(BIG, p)
        out.append((d, synth.box_room_color(BIG, p, d), p))
    return out


def _add_frame(r, fid, frame):
    """gaussians_add alone, as Mapping.mapping enters it."""
    m, (d, c, c2w) = r.f, frame
    fr = mp.Frame(BIG, c2w, DEV, uid=fid)
    fm = rp.frame_maps(DEV)(d, c, c2w, BIG, m.args)
    fm["color_chw"] = fm["color_map"].permute(2, 0, 1).contiguous()
    fm["depth_chw"] = fm["depth_map"].permute(2, 0, 1).contiguous()
    m.frame_map = fm
    m.gaussians_add(fr)
    m.time += 1
    return m.stats.get("last_add")


def _count_calls(ops):
    calls = dict(n=0)
    inner = ops.knn_stable

    def knn_stable(*a):
        calls["n"] += 1
        return inner(*a)
    ops.knn_stable = knn_stable
    return calls


@functools.lru_cache(maxsize=None)
def _first_frame_counts():
    """(candidates, kept by the filter, accepted) of frame 1 on the seeded map: the draw is keyed by args.seed, so every Mapping
    seeded the same way sees the same counts."""
    args = _big_args()
    from types import SimpleNamespace
    return _add_frame(SimpleNamespace(f=_seeded(3000, 60000, args)), 0, _big_frames(1)[0])


@functools.lru_cache(maxsize=None)
def _stable_freeze():
    """21 000 stable rows: temp_to_optimize searches through knn_stable.  Two frames reuse ONE structure (frozen_key stands: the
    appends fit the capacity and touch no frozen row); a gaussians_fix changes the key and the third frame builds again.  On
    every frame the appended rows equal the tensor form's, whose neighbours come from rtgs_knn3_query over cat(new, map)."""
    args = _big_args()
    m = _seeded(3000, 60000, args)
    calls = _count_calls(m.ops)
    r = rp.Replay(m, mp.HipOps(args, DEV), bookkeeping=False, defer_tolerances=True)
    frames = _big_frames(3)
    builds = []
    for fid in (0, 1):
        la = _add_frame(r, fid, frames[fid])
        assert la is not None and la[2] > 100 and la[2] < la[1], la              # rows were accepted, and some were refused
        builds.append(m.ops.stable_builds)
    assert builds == [1, 1] and calls["n"] == 2
    key = m.opt.frozen_key
    mask = torch.zeros(m.opt.n_train, dtype=torch.bool, device=DEV)
    mask[::7] = True
    m.gaussians_fix(mask=mask)
    assert m.opt.frozen_key != key and m.opt.n_frozen == N_STABLE + int(mask.sum())
    la = _add_frame(r, 2, frames[2])
    builds.append(m.ops.stable_builds)
    assert la is not None and la[2] > 0 and builds == [1, 1, 2] and calls["n"] == 3
    assert r.seen["adds"] == 3 and r.render_checked
    margins.record("stable_search", stable_builds=builds, rows_added=r.seen["rows"], frames=3)
    return r.seen


def test_the_stable_structure_is_built_once_and_rebuilt_after_a_freeze():
    _stable_freeze()


@functools.lru_cache(maxsize=None)
def _stable_realloc():
    """The capacity holds frame 1's candidates exactly; frame 2's append_rows_masked has to reallocate: the arrays move,
    frozen_key changes, frame 3 searches a rebuilt structure - and every frame's rows still equal the tensor form's."""
    args = _big_args()
    n_all, n1, m1 = _first_frame_counts()
    m = _seeded(3000, N_STABLE + 3000 + n1, args)
    calls = _count_calls(m.ops)
    r = rp.Replay(m, mp.HipOps(args, DEV), bookkeeping=False, defer_tolerances=True)
    frames = _big_frames(3)
    ptrs, builds = [m.opt.state["xyz"]["p"].data_ptr()], []
    for fid in range(3):
        la = _add_frame(r, fid, frames[fid])
        assert la is not None and la[2] > 0, la
        ptrs.append(m.opt.state["xyz"]["p"].data_ptr())
        builds.append(m.ops.stable_builds)
    assert ptrs[1] == ptrs[0] and ptrs[2] != ptrs[1], "frame 2's append did not reallocate"
    assert builds == [1, 1, 2] and calls["n"] == 3 and r.seen["adds"] == 3
    margins.record("stable_search", stable_builds=builds, rows_added=r.seen["rows"], frames=3)
    return r.seen


def test_the_stable_structure_is_rebuilt_after_a_reallocation():
    _stable_realloc()


@functools.lru_cache(maxsize=None)
def _stable_decline():
    """31 000 unstable rows and a frame that draws about 3 500 points: new + unstable > 32 768, the guard in temp_to_optimize
    keeps the one-structure query."""
    args = _big_args(6000)
    m = _seeded(31000, 70000, args)
    calls = _count_calls(m.ops)
    r = rp.Replay(m, mp.HipOps(args, DEV), bookkeeping=False, defer_tolerances=True)
    la = _add_frame(r, 0, _big_frames(1)[0])
    assert la is not None and la[1] + 31000 > 32768 and la[2] > 0, la
    assert calls["n"] == 0 and m.ops.stable_builds == 0 and r.seen["adds"] == 1
    margins.record("stable_search", stable_builds=[0], rows_added=r.seen["rows"], frames=1)
    return r.seen


def test_the_stable_search_declines_past_32768_directly_compared_points():
    _stable_decline()


RUNS = {"stream-7": lambda: _lifecycle(7, False), "changing-15": lambda: _lifecycle(15, True),
        "three-in-the-error-pass": lambda: _lifecycle(7, False, THREE[0]), "three-in-the-transmission-pass": lambda: _lifecycle(7, False, THREE[1]),
        "stable-freeze": _stable_freeze, "stable-reallocation": _stable_realloc, "stable-declined": _stable_decline}


@pytest.mark.parametrize("run", list(RUNS))
def test_rotations_and_raw_scales_of_the_appended_rows(run):
    """The two toleranced columns of every replayed run above: rotations and raw scales of the appended rows within 2e-6 of the
    tensor form's - the bound tests/test_slam_ops_gpu.py holds the same kernels to on random normals.

    MEASURED on the MI355X: rotations 0 on all seven runs (514 / 871 / 523 / 271 / 1967 / 1963 / 2555 appended rows), raw scales
    at most 1.43e-6.  Before mapping.unit_normals the rotations MISSED the bound on five runs (2.4e-6 .. 8.1e-6 on single rows):
    the box room's walls face the camera, |n_z| is within 1e-5 .. 5e-4 of 1, and d acos / d n_z = 1 / sqrt(1 - n_z^2) turns one
    ulp of the unit normal into up to 1e-5 of the quaternion.  The kernel's normal equals sqrt((x x + y y) + z z) without
    contraction on every row, torch.norm on the device rounded its sum differently on about 8 % of them; against the float64
    rotation both were off by the same 2.8e-6 .. 1.2e-5, so neither was the wrong one - the tensor form on the device now
    spells the sum out as the kernel does."""
    rp.assert_tolerances(RUNS[run]())


# ---------------------------------------------------------------------------------------------------------------- d. one workgroup
SIZES = [1023, 1024, 1025, 65535, 65536, 65537, 100000]


def _keep(n, ratio, gen):
    if ratio in (0.0, 1.0):
        return torch.full((n,), bool(ratio))
    return torch.rand(n, generator=gen) < ratio


@pytest.mark.parametrize("n", SIZES)
def test_compact_points_and_bbox_pad_at_and_past_a_chunk_and_64_chunks(n):
    from rtg_slam_amd import slam_ops
    gen = torch.Generator().manual_seed(n)
    xyz, col = torch.randn(n, 3, generator=gen).to(DEV), torch.rand(n, 3, generator=gen).to(DEV)
    opa, rot = torch.randn(n, 1, generator=gen).to(DEV), torch.randn(n, 4, generator=gen).to(DEV)
    box = slam_ops.bbox_pad(xyz, 0.05)
    assert torch.equal(box, torch.cat([xyz.min(dim=0)[0] - 0.05, xyz.max(dim=0)[0] + 0.05]))
    for ratio in (0.0, 1.0, 0.5):
        keep = _keep(n, ratio, gen).to(DEV)
        cx, cc, co, cr, m = slam_ops.compact_points(keep, xyz, col, opa, rot)
        assert m == int(keep.sum()) and (ratio != 0.5 or 0 < m < n)
        assert torch.equal(cx, xyz[keep]) and torch.equal(cc, col[keep]) and torch.equal(co, opa[keep]) and torch.equal(cr, rot[keep])


@pytest.mark.parametrize("n", SIZES)
def test_append_rows_masked_at_and_past_a_chunk_and_64_chunks(n):
    gen = torch.Generator().manual_seed(n + 1)
    base = torch.randn(300, mo.COLS, generator=gen).to(DEV)
    rows = torch.randn(n, mo.COLS, generator=gen).to(DEV)
    for ratio in (0.0, 1.0, 0.5):
        valid = _keep(n, ratio, gen).to(torch.uint8).to(DEV)
        maps = []
        for masked in (False, True):
            o = mo.ShardedMapOptimizer(base.clone(), lr_col=mo.default_lr_columns(), capacity=400)
            for name, dtype, fill in AUX:
                o.add_aux(name, 1, dtype, fill)
            if masked:
                m = o.append_rows_masked(rows, valid, aux={"add_tick": 41})
            else:
                good = torch.nonzero(valid).reshape(-1)
                m = int(good.shape[0])
                if m:
                    o.append_rows(rows[good], aux={"add_tick": 41})
            assert m == int(valid.sum()) and o.N == 300 + m
            maps.append(o)
        a, b = maps
        assert torch.equal(a.params, b.params)
        for name, _, _ in AUX:
            assert torch.equal(a.aux[name][:a.N], b.aux[name][:b.N]), name


def _delete_inputs(n, time_now=250, window=120):
    """Radii of 0.002 .. 0.012 and forty giants fifty times the mean: nothing near 10 x mean - checked on the CPU."""
    gen = torch.Generator().manual_seed(n)
    scales = 0.002 + 0.01 * torch.rand(n, 3, generator=gen)
    scales[torch.randperm(n, generator=gen)[:40]] *= 50
    tick = torch.randint(0, 300, (n,), generator=gen, dtype=torch.int32)
    want, band, thr = rp.delete_reference(scales, tick, time_now, window)
    r = rp.radius32(scales).double()
    assert int(band.sum()) == 0 and float(((r - thr).abs() / thr).min()) > 1e-3 and int((r > thr).sum()) == 40
    return scales, tick, want


@pytest.mark.parametrize("n", [65535, 65536])
def test_delete_mask_at_its_largest_cloud(n):
    from rtg_slam_amd import slam_ops
    scales, tick, want = _delete_inputs(n)
    mask, k = slam_ops.delete_mask(scales.to(DEV), tick.to(DEV), 250, 120)
    assert torch.equal(mask.bool().cpu(), want) and k == int(want.sum()) and 40 < k < n
    big = rp.delete_reference(scales, None, 0, 0)[0]
    mask, k = slam_ops.delete_mask(scales.to(DEV), None, 250, 120)
    assert torch.equal(mask.bool().cpu(), big) and k == 40


def test_gaussians_delete_past_65536_unstable_rows_takes_the_tensor_branch():
    """65 537 unstable rows: Mapping.gaussians_delete leaves the single-workgroup kernel alone.  Its survivors are those of the
    kernel's path on the first 65 536 rows - the extra row is too old and goes (no radius is near 10 x either mean)."""
    n = 65537
    scales, tick, want = _delete_inputs(n)
    tick[n - 1] = 0                                                       # 250 - 0 > 120
    want = rp.delete_reference(scales, tick, 250, 120)[0]
    want_head, band_head, _ = rp.delete_reference(scales[:n - 1], tick[:n - 1], 250, 120)
    assert torch.equal(want[:n - 1], want_head) and int(band_head.sum()) == 0 and bool(want[n - 1])
    g = synth.surface_gaussians(n, BIG, seed=2)
    g["scales"] = scales
    packed = mo.pack_from_activated({k: v.to(DEV) for k, v in g.items()})
    args = tm._args(unstable_time_window=120)
    out = []
    for rows in (n, n - 1):
        m = mp.Mapping(args, DEV, capacity=8)
        calls = dict(n=0)
        inner = m.ops.delete_mask

        def delete_mask(*a, _inner=inner, _calls=calls, **kw):
            _calls["n"] += 1
            return _inner(*a, **kw)
        m.ops.delete_mask = delete_mask
        opt = mo.ShardedMapOptimizer(packed[:rows].clone(), lr_col=m.lr_col, n_frozen=0, capacity=rows)
        for name, dtype, fill in AUX:
            opt.add_aux(name, 1, dtype, fill)
        opt.aux["add_tick"][:rows, 0] = tick[:rows].to(DEV)
        m.opt, m.time = opt, 250
        m.gaussians_delete()
        assert calls["n"] == (0 if rows == n else 1)
        assert m.stats["deleted_unstable"] == int(want[:rows].sum()) and m.opt.N == rows - int(want[:rows].sum())
        assert torch.equal(m.opt.params, packed[:rows][~want[:rows].to(DEV)])
        out.append(m.opt.params)
    assert torch.equal(out[0], out[1])
