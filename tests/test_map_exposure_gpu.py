"""csrc/map_exposure.hip and rtg_slam_amd/map_exposure.py against their definition, tests/map_exposure_reference.py: the eight
float64 sums and the state bit for bit after every iteration, the cases of tests/test_map_exposure_cpu.py through the kernels, the
corrected colour in both layouts, the mapper on a short sequence whose frames change exposure, and the defaults untouched."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import map_exposure_reference as mer
from tests import test_map_exposure_cpu as cpu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
NEW_ENTRIES = ("rtgs_map_exposure_fit", "rtgs_map_exposure_apply", "rtgs_map_exposure_scratch_bytes")
NAMES = ("frame_color", "frame_depth", "render_color", "render_depth", "T_map")
# [H, W]: four chunks and a tail of 704; exactly two chunks; one pixel short of a chunk; one pixel over a chunk; one pixel
SIZES = [(60, 80), (32, 64), (31, 33), (25, 41), (1, 1)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def stage(**over):
    from rtg_slam_amd import map_exposure as me
    return me.MapExposure(SimpleNamespace(**{"map_exposure_" + k: v for k, v in over.items()}), DEV)


def run(s, start=(1.0, 0.0), iters=4, **over):
    """The kernels, one iteration at a time -> the host copy of the state after each."""
    from rtg_slam_amd import map_exposure as me
    m = stage(iters=iters, **over)
    m.state[0], m.state[1] = start
    d = [dev(s[k]) for k in NAMES]
    out = []
    for k in range(iters):
        m.fit_iteration(*d, k)
        out.append(m.state.cpu().numpy().copy())
    assert me.SUMS_AT == 8 and me.STATE == 16
    return out


def assert_matches(states, steps, start):
    for k, (st, (S, alpha, beta, code)) in enumerate(zip(states, steps)):
        assert np.array_equal(bits(st[8:16]), bits(S)), (k, st[8:16], S)
        assert np.array_equal(bits(st[:2]), bits([alpha, beta])), (k, st[:2], alpha, beta)
        assert st[4] == code, (k, st[4], code)
        assert np.array_equal(bits(st[2:4]), bits(start))


@pytest.mark.parametrize("start", [(1.0, 0.0), (0.8, 0.05)])
@pytest.mark.parametrize("H,W", SIZES)
def test_sums_and_state_match_the_definition_after_every_iteration(H, W, start):
    s = mer.gated_scene(H, W)
    over = {"min_valid": 1} if H * W == 1 else {}
    states = run(s, start, **over)
    _, code, steps = mer.fit(**s, state=start, **over)
    assert_matches(states, steps, start)
    assert code == (mer.FLAT if H * W == 1 else mer.OK)
    if H * W == 1:                                                              # and with the default min_valid it is too few
        states = run(s, start)
        _, code, steps = mer.fit(**s, state=start)
        assert code == mer.TOO_FEW
        assert_matches(states, steps, start)


def test_two_runs_are_bit_equal_and_refusals_launch_nothing():
    from rtg_slam_amd import _lib
    s = mer.gated_scene(60, 80)
    a, b = run(s, (0.8, 0.05)), run(s, (0.8, 0.05))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
    lib = _lib.load()
    for H, W in SIZES + [(680, 1200)]:
        assert lib.rtgs_map_exposure_scratch_bytes(H, W) == -(-H * W // 1024) * 8 * 8
    for H, W in ((0, 80), (60, 0), (-1, 80), (65536, 65536), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.rtgs_map_exposure_scratch_bytes(H, W) == 0
    E = _lib.CONSTANTS["RTGS_E_INVALID"]
    m = stage()
    m.state[0], m.state[1] = 0.7, 0.1
    before = m.state.clone()
    d = [dev(s[k]) for k in NAMES]
    scratch = torch.empty(lib.rtgs_map_exposure_scratch_bytes(60, 80) // 8, dtype=torch.float64, device=DEV)
    out = torch.empty(2, 3 * 60 * 80, dtype=torch.float32, device=DEV)
    p, st = _lib.ptr, _lib.stream(DEV)
    good = [p(t) for t in d] + [60, 80, 0, 0.05, 3.0, 0.05, 0.1, 4 / 255, 251 / 255, 1e-4, 64, p(m.state), p(scratch), st]
    for i in (0, 1, 2, 3, 4, 16, 17):                                           # a null pointer
        bad = list(good)
        bad[i] = None
        assert lib.rtgs_map_exposure_fit(*bad) == E
    for i, v in ((5, 0), (6, 0), (5, 65536), (7, -1), (8, 0.0), (8, float("nan")), (9, 0.5), (10, -1.0), (12, 0.99), (14, -1.0),
                 (15, 0)):
        bad = list(good)
        bad[i] = v
        if (i, v) == (5, 65536):
            bad[6] = 65536
        assert lib.rtgs_map_exposure_fit(*bad) == E, (i, v)
    ok = [p(d[0]), 60, 80, p(m.state), p(out[0]), p(out[1]), st]
    for i, v in ((0, None), (3, None), (4, None), (5, None), (1, 0), (2, -3), (4, p(d[0]))):
        bad = list(ok)
        bad[i] = v
        assert lib.rtgs_map_exposure_apply(*bad) == E, (i, v)
    torch.cuda.synchronize()
    assert torch.equal(m.state, before)


@pytest.mark.parametrize("gain,offset", mer.RECOVERY_CASES)
def test_recovery_through_the_kernels(gain, offset):
    s = mer.scene(60, 80, gain, offset)
    states = run(s)
    state, code, steps = mer.fit(**s)
    assert_matches(states, steps, (1.0, 0.0))
    assert code == mer.OK and cpu.off(states[-1][:2], gain, offset) <= cpu.RECOVERY_TOL


@pytest.mark.parametrize("seed", mer.ROBUST_SEEDS)
def test_robustness_through_the_kernels(seed):
    g, o = cpu.ROBUST_CASE
    s = mer.scene(60, 80, g, o, outliers=0.2, seed=seed)
    sched = run(s)
    assert_matches(sched, mer.fit(**s)[2], (1.0, 0.0))
    plain = run(s, cut=1e30)                                                     # a cut no residual reaches: four Huber iterations
    assert_matches(plain, mer.fit(**s, weight_fn=cpu.huber_only)[2], (1.0, 0.0))
    assert cpu.off(sched[-1][:2], g, o) <= cpu.SCHEDULE_BOUND and cpu.off(plain[-1][:2], g, o) > cpu.HUBER_BOUND


@pytest.mark.parametrize("name", ["constant frame", "too few valid pixels", "gain 5"])
def test_fallbacks_through_the_kernels(name):
    s, want = cpu.fallback_scenes()[name]
    states = run(s, cpu.START)
    _, code, steps = mer.fit(**s, state=cpu.START)
    assert_matches(states, steps, cpu.START)
    assert code == want and all(st[4] == want and tuple(st[:2]) == cpu.START and st[5] == 0 for st in states)


def test_history_is_one_record_per_frame():
    m = stage()
    m.skip()
    s = mer.scene(60, 80, 1.25, -0.06)
    bad, _ = cpu.fallback_scenes()["constant frame"]
    for sc in (s, bad):
        m.fit(dev(sc["frame_color"]), dev(sc["frame_depth"]),
              {"render": dev(sc["render_color"]), "depth": dev(sc["render_depth"]), "T_map": dev(sc["T_map"])})
    h = m.history()
    want, _, steps = mer.fit(**s)
    assert h[0] == (1.0, 0.0, 0, 0, 0)
    assert h[1] == (want[0], want[1], 0, int(steps[-1][0][6]), int(steps[-1][0][7]))
    assert h[2][:3] == (want[0], want[1], mer.FLAT) and h[2][3] == 4800          # fell back to the previous frame's state
    rep = m.report()
    assert rep["frames_fitted"] == 2 and rep["frames_fell_back"] == 1 and rep["fell_back"] == {"2": "no variance of intensity"}
    assert rep["options"]["huber"] == 0.05 and rep["options"]["iters"] == 4


def test_apply_writes_both_layouts_into_new_storage():
    rng = np.random.default_rng(7)
    c = rng.random((3, 37, 53)).astype(F32)
    c[0, 0, :4] = (0.0, 1.0, 0.5, 0.999)
    for alpha, beta in ((1.3, -0.1), (0.8, 0.3), (1.0, 0.0)):
        m = stage()
        m.state[0], m.state[1] = alpha, beta
        t = dev(c)
        chw, hwc = m.apply(t)
        want_chw, want_hwc = mer.apply(c, alpha, beta)
        assert np.array_equal(bits32(chw.cpu().numpy()), bits32(want_chw))
        assert np.array_equal(bits32(hwc.cpu().numpy()), bits32(want_hwc))
        assert chw.shape == (3, 37, 53) and hwc.shape == (37, 53, 3) and chw.is_contiguous() and hwc.is_contiguous()
        assert np.array_equal(t.cpu().numpy(), c)                                # the input is not written
        assert len({t.data_ptr(), chw.data_ptr(), hwc.data_ptr()}) == 3
    chw, _ = mer.apply(c, 1.3, -0.1)
    assert (chw == 0).any() and (chw == 1).any()                                 # the clamp is active at both ends


# ---- the mapper ----

FRAMES = 12
GAINS = [(1.0, 0.0)] + [((1.2, -0.03) if k % 2 else (0.85, 0.02)) for k in range(1, FRAMES)]


def _cam():
    from rtg_slam_amd import synth
    return synth.CameraSpec(240, 320, 160.0, 160.0, 159.5, 119.5)


def _args(**over):
    from rtg_slam_amd import mapping as mp
    kw = dict(uniform_sample_num=4000, gaussian_update_iter=30, max_depth=8.0, keyframe_trans_thes=0.03, seed=1, use_gt_pose=True)
    kw.update(over)
    return mp.replica_args(**kw)


_clean = {}


def _frames(n):
    """The box room along synth.trajectory at GT poses: (depth, clean colour, c2w), computed once."""
    from rtg_slam_amd import synth
    cam = _cam()
    if n not in _clean:
        out = []
        for p in synth.trajectory(n, seed=21):
            d = synth.box_room_depth(cam, p)
            out.append((d.to(DEV), synth.box_room_color(cam, p, d).to(DEV), p.numpy()))
        _clean[n] = out
    return _clean[n]


def _run(args, gains=None, n=FRAMES):
    """-> (mapper, report, the colour tensors handed in, per frame what frame_map held after mapping, mean |render - clean|)."""
    from rtg_slam_amd import slam
    frames = _frames(n)
    given, seen, views = [], [], []
    torch.manual_seed(1)                                                         # the pixel sampler draws from torch's generator

    def stream():
        for k, (d, c, c2w) in enumerate(frames):
            if gains is not None:
                c = (c * gains[k][0] + gains[k][1]).clamp_(0.0, 1.0)
            given.append(c)
            yield d, c, c2w

    def on_frame(frame_id, frame, frame_map, mapper, tracker):
        seen.append({k: frame_map.get(k) for k in ("color_chw", "color_map", "color_raw_chw")})
        views.append(frame)

    mapper, tracker, rep = slam.run_sequence(_cam(), stream(), args, DEV, capacity=100_000, on_frame=on_frame)
    err = torch.stack([(mapper._render(f, "all")["render"] - frames[k][1]).abs().mean() for k, f in enumerate(views)]).mean()
    return mapper, tracker, rep, given, seen, float(err)


def test_mapper_keeps_the_map_in_one_exposure():
    """Twelve box-room frames at GT poses, so that only colour differs.  Mean absolute colour error of the final map, rendered at
    the twelve poses, against the clean colour - printed for the three runs; the option must make it smaller.  On an MI355X:
    0.0031 on the clean stream, 0.0132 with the gains and the option off, 0.0057 with it on; alpha 0.819-0.823 for 1 / 1.2 = 0.833
    and 1.158-1.162 for 1 / 0.85 = 1.176."""
    _, _, _, _, _, e_clean = _run(_args())
    _, _, rep_off, _, seen_off, e_off = _run(_args(), GAINS)
    mapper, _, rep, given, seen, e_on = _run(_args(map_exposure=True), GAINS)
    hist = mapper.map_exposure.history()
    print(f"map colour error against the clean colour: clean stream {e_clean:.5f}, gains with the option off {e_off:.5f}, on {e_on:.5f}")
    print("alpha per frame:", [round(h[0], 4) for h in hist], "for 1 / gain", [round(1 / g, 4) for g, _ in GAINS])
    print("beta per frame:", [round(h[1], 4) for h in hist], "for -offset / gain", [round(-o / g, 4) for g, o in GAINS])
    assert e_on < e_off
    assert len(hist) == FRAMES and hist[0] == (1.0, 0.0, 0, 0, 0)
    for k in range(1, FRAMES):
        alpha, beta, code, valid, inliers = hist[k]
        assert code == 0, (k, hist[k])                                           # no frame falls back
        assert abs(alpha - 1 / GAINS[k][0]) < abs(1 - 1 / GAINS[k][0]), (k, alpha)
        assert valid >= 240 * 320 // 100
    assert rep["map_exposure"]["frames_fitted"] == FRAMES - 1 and rep["map_exposure"]["frames_fell_back"] == 0
    assert "map_exposure" not in rep_off and all(s["color_raw_chw"] is None for s in seen_off)
    for k in range(FRAMES):
        assert seen[k]["color_raw_chw"] is given[k]                              # the stream's tensor, untouched
        assert torch.equal(given[k], (_frames(FRAMES)[k][1] * GAINS[k][0] + GAINS[k][1]).clamp(0, 1))
        if k > 0:
            assert seen[k]["color_chw"].data_ptr() != given[k].data_ptr()
            assert torch.equal(seen[k]["color_map"], seen[k]["color_chw"].permute(1, 2, 0))
            near = (seen[k]["color_chw"] - _frames(FRAMES)[k][1]).abs().mean()
            assert float(near) < float((given[k] - _frames(FRAMES)[k][1]).abs().mean())
    # the keyframe copies hold the corrected colour
    assert len(mapper.keymap_list) >= 2
    for km in mapper.keymap_list:
        k = int(km["time"])
        assert km["color_chw"] is seen[k]["color_chw"] and km["color_map"] is seen[k]["color_map"]


def test_off_means_off(monkeypatch):
    """Bit-equality of two runs can only be asked where the project's own runs are reproducible: with optimisation steps the
    rasterizer's backward adds gradients in arrival order, and two runs of the same arguments WITHOUT the key already differ (on an
    MI355X 4 308 against 4 324 Gaussians after these six frames; DESIGN.md: "the sequence is not deterministic, atomics decide a
    few hundred Gaussians").  So the six frames run with gaussian_update_iter = 0 - every frame still renders the model, builds
    the add masks, draws, filters and appends new Gaussians, fixes and deletes: the whole path the option hooks into."""
    from rtg_slam_amd import _lib
    lib = _lib.load()
    calls = {n: 0 for n in NEW_ENTRIES}

    def counted(name, fn):
        def wrapper(*a):
            calls[name] += 1
            return fn(*a)
        return wrapper

    for name in NEW_ENTRIES:
        monkeypatch.setattr(lib, name, counted(name, getattr(lib, name)))
    absent = _args(gaussian_update_iter=0)
    assert not hasattr(absent, "map_exposure")
    m_a, t_a, rep_a, given_a, seen_a, _ = _run(absent, GAINS, n=6)
    m_b, t_b, rep_b, _, _, _ = _run(_args(gaussian_update_iter=0), GAINS, n=6)
    m_f, t_f, rep_f, _, seen_f, _ = _run(_args(gaussian_update_iter=0, map_exposure=False), GAINS, n=6)
    assert m_a.opt.N > 4000 and m_a.stats["added"] > m_a.stats["added"] - m_a.opt.N >= 0
    assert calls == {n: 0 for n in NEW_ENTRIES}
    for m, t, rep in ((m_b, t_b, rep_b), (m_f, t_f, rep_f)):
        assert m.map_exposure is None and "map_exposure" not in rep
        assert np.array_equal(np.stack(t.pose_es), np.stack(t_a.pose_es))
        print("Gaussians of the two runs:", m.opt.N, m_a.opt.N)
        assert m.opt.N == m_a.opt.N
        assert torch.equal(m.opt.params[:m.opt.N], m_a.opt.params[:m_a.opt.N])
    for k in range(6):                                                           # frame_map holds the tensors it always held
        assert seen_a[k]["color_chw"] is given_a[k] and seen_a[k]["color_raw_chw"] is None
    _run(_args(map_exposure=True), GAINS, n=6)
    assert calls["rtgs_map_exposure_fit"] == 5 * 4 and calls["rtgs_map_exposure_apply"] == 5
