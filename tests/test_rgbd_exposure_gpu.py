"""csrc/rgbd_exposure.hip and the exposure / model-target paths of rtg_slam_amd/rgbd_align.py and slam.Tracker against their
definition, tests/rgbd_exposure_reference.py: the 48 float64 sums and the composite target's pyramid bit for bit, the
eight-unknown loop's pose and exposure bit for bit, the tracker on a wall whose frames change exposure, and the defaults
untouched."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rgbd_align_reference as ref
from tests import rgbd_exposure_reference as rer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DIST, COS = 0.1, float(np.cos(np.deg2rad(20.0)))
NAMES = ("v_src", "n_src", "i_src", "v_tgt", "n_tgt", "i_tgt")
NEW_ENTRIES = ("rtgs_rgbd_align_accumulate_exposure", "rtgs_rgbd_align_exposure_scratch_bytes", "rtgs_rgbd_target_intensity")
EXPOSURES = [(1.0, 0.0), (0.8, 0.048), (1.25, -0.1)]
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


_scenes = {}


def scene(H, W):
    """The flat textured wall pair with every gate exercised: holes in the target depth, source pixels without a normal (the
    geometric gate fails where the photometric one passes), source rows without depth, a NaN vertex."""
    if (H, W) not in _scenes:
        s = ref.wall_pair(H, W)
        s["v_tgt"][H // 6:H // 6 + 4, W // 4:W // 4 + 10] = 0
        s["n_src"][H // 2:H // 2 + 5, W // 16:W // 16 + 20] = 0
        s["v_src"][2 * H // 3:2 * H // 3 + 2] = 0
        s["v_src"][5, 7] = np.nan
        s["dev"] = {k: dev(s[k]) for k in NAMES}
        _scenes[(H, W)] = s
    return _scenes[(H, W)]


def poses(W):
    """The second slides the source by 85 % of the wall's visible width (W / f times the 2 m of depth): most pixels leave the view."""
    return {"identity": np.eye(4),
            "mostly out of view": ref.se3_exp(np.array([0.0, 0.0, 0.0, 0.85 * W * ref.WALL_Z / 70.0, 0.0, 0.0]))}


def both(s, pose, alpha, beta, photo_weight=0.25, huber=0.05, over=None):
    from rtg_slam_amd import rgbd_align
    host = {k: s[k] for k in NAMES}
    d = dict(s["dev"])
    for k, v in (over or {}).items():
        host[k], d[k] = v, dev(v)
    want = rer.accumulate(*[host[k] for k in NAMES], s["K"], pose, DIST, COS, photo_weight, huber, alpha, beta)
    run = lambda: rgbd_align.accumulate_exposure(*[d[k] for k in NAMES], dev(s["K"]), dev(pose.astype(np.float32)), DIST, COS,
                                                 photo_weight, huber, alpha, beta).cpu().numpy()
    return want, run(), run()


def check_sums(H, W, pose, alpha, beta):
    s = scene(H, W)
    want, got, again = both(s, poses(W)[pose], alpha, beta)
    n = H * W
    print(f"{W}x{H} {pose} ({alpha}, {beta}): geometric {want[45]:.0f} photometric {want[47]:.0f} of {n}")
    assert want.shape == (48,) and got.shape == (48,)
    if pose == "mostly out of view":
        assert 6 <= want[47] < 0.25 * n
    else:
        assert want[47] > 0.5 * n and 0 < want[45] < want[47]
    assert np.array_equal(bits(got), bits(want)), (got - want)
    assert np.array_equal(bits(got), bits(again))


# 15 x 20: one chunk, slots with 0, 1 or 2 pixels; 30 x 40: two chunks, the second ragged; 60 x 80: 4.69 chunks
@pytest.mark.parametrize("alpha,beta", EXPOSURES)
@pytest.mark.parametrize("pose", list(poses(80)))
@pytest.mark.parametrize("H,W", [(15, 20), (30, 40), (60, 80)])
def test_sums_are_the_definitions_bit_for_bit(H, W, pose, alpha, beta):
    check_sums(H, W, pose, alpha, beta)


def test_sums_over_300_chunks():
    """480 x 640: the only case in which `total`'s slots add more than one chunk row."""
    check_sums(480, 640, "identity", 0.8, 0.048)


def test_unit_exposure_is_the_six_unknown_kernel():
    from rtg_slam_amd import rgbd_align
    s = scene(60, 80)
    pose = ref.se3_exp(ref.WALL_XI)
    d = s["dev"]
    six = rgbd_align.accumulate(*[d[k] for k in NAMES], dev(s["K"]), dev(pose.astype(np.float32)), DIST, COS, 0.25, 0.05).cpu().numpy()
    _, eight, _ = both(s, pose, 1.0, 0.0)
    assert np.array_equal(bits(rer.pose_block(eight)), bits(six))


def test_sums_without_source_depth_are_plus_zero():
    s = scene(60, 80)
    want, got, again = both(s, ref.se3_exp(ref.WALL_XI), 0.8, 0.048, over={"v_src": np.zeros_like(s["v_src"])})
    assert np.array_equal(bits(want), np.zeros(48, np.int64))
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got), bits(again))


@pytest.mark.parametrize("alpha,beta", EXPOSURES)
def test_sums_with_both_huber_branches(alpha, beta):
    s = scene(60, 80)
    huber = 0.01
    t = rer.pixel_terms(*[s[k] for k in NAMES], s["K"], poses(80)["identity"], DIST, COS, 0.25, huber, alpha, beta)
    r = np.abs(t["rI"][t["photo"]])
    print(f"({alpha}, {beta}): {(r > huber).sum()} pixels above the Huber threshold, {(r <= huber).sum()} at or below")
    assert (r > huber).sum() > 100 and (r <= huber).sum() > 100
    want, got, again = both(s, poses(80)["identity"], alpha, beta, huber=huber)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got), bits(again))


def test_sums_with_photo_weight_zero():
    s = scene(60, 80)
    want, got, _ = both(s, ref.se3_exp(ref.WALL_XI), 1.25, -0.1, photo_weight=0.0)
    assert want[45] > 0 and want[0] > 0 and not want[[6, 7, 33, 34, 35]].any()    # the pose block is geometric, rows 6 and 7 empty
    assert np.array_equal(bits(got), bits(want))


def test_loop_is_the_definitions_bit_for_bit_and_recovers_the_wall():
    from rtg_slam_amd import rgbd_align
    s = rer.exposed_wall_pair(60, 80, 1.25, -0.06)
    d = {k: dev(s[k]) for k in NAMES}
    truth = s["truth"]
    args = SimpleNamespace(rgbd_refine_iters=[12], icp_distance_threshold=DIST, icp_normal_threshold=20.0, rgbd_refine_exposure=True)
    T, rep = rgbd_align.RgbdRefiner(args).refine(np.eye(4), *[[d[k]] for k in NAMES], dev(s["K"]), [1.0])
    T_ref, rep_ref = rer.refine(np.eye(4), *[[s[k]] for k in NAMES], s["K"], [1.0], iters=[12], distance_threshold=DIST,
                                cos_threshold=COS)
    assert rep["iterations"] == rep_ref["iterations"] and rep["rank"] == rep_ref["rank"] and rep["reason"] == rep_ref["reason"]
    assert rep["inliers_photometric"] == rep_ref["inliers_photometric"] and rep["inliers_geometric"] == rep_ref["inliers_geometric"]
    assert rep["exposure"] == rep_ref["exposure"] and rep["exposure_steps"] == rep_ref["exposure_steps"]
    assert np.array_equal(bits(T), bits(T_ref))
    before, after = np.linalg.norm(truth[:3, 3]), np.linalg.norm(T[:3, 3] - truth[:3, 3])
    print(f"refined: {1e3 * before:.2f} mm -> {1e3 * after:.3f} mm, exposure {rep['exposure']}, rank {rep['rank']}, "
          f"device {1e3 * rep['device_s']:.3f} ms, {rep['host_reads']} host reads")
    assert after <= 0.05 * before
    assert rep["host_reads"] == len(rep["inliers_photometric"]) and rep["device_s"] > 0
    # and an explicit start is the definition's too
    T2, rep2 = rgbd_align.RgbdRefiner(args).refine(np.eye(4), *[[d[k]] for k in NAMES], dev(s["K"]), [1.0], exposure=(0.8, 0.05))
    T2_ref, rep2_ref = rer.refine(np.eye(4), *[[s[k]] for k in NAMES], s["K"], [1.0], iters=[12], distance_threshold=DIST,
                                  cos_threshold=COS, exposure=(0.8, 0.05))
    assert np.array_equal(bits(T2), bits(T2_ref)) and rep2["exposure"] == rep2_ref["exposure"]


def target_case(H, W, seed):
    rng = np.random.default_rng(seed)
    render, frame = rng.random((3, H, W)).astype(F32), rng.random((3, H, W)).astype(F32)
    rendered = (1 + rng.random((H, W))).astype(F32)
    rendered[H // 4:H // 2, W // 3:W // 2] = 0
    filled = rendered.copy()
    filled[H // 4:H // 2, W // 3:W // 2] = (2 + rng.random((H // 2 - H // 4, W // 2 - W // 3))).astype(F32)
    mask = rng.random((H, W)) < 0.1                                           # scattered replacements too
    filled[mask] = (3 + rng.random(int(mask.sum()))).astype(F32)
    return render, frame, rendered, filled


@pytest.mark.parametrize("H,W", [(60, 80), (61, 83)])
def test_target_intensity_is_the_definitions(H, W):
    from rtg_slam_amd import rgbd_align
    render, frame, rendered, filled = target_case(H, W, H)
    for alpha, beta in ((1.0, 0.0), (0.8, 0.05)):
        want = rer.target_intensity_pyramid(render, frame, rendered, filled, alpha, beta, 3)
        got = rgbd_align.target_intensity_pyramid(dev(render), dev(frame), dev(rendered), dev(filled), alpha, beta, 3)
        assert [tuple(g.shape) for g in got] == [w.shape for w in want]
        for g, w in zip(got, want):
            assert np.array_equal(bits32(g.cpu().numpy()), bits32(w))
        # [H,W,3] colours and [H,W,1] depths, as the mapper's render output has them
        hwc = rgbd_align.target_intensity_pyramid(dev(render).permute(1, 2, 0), dev(frame.transpose(1, 2, 0)), dev(rendered)[..., None],
                                                  dev(filled)[..., None], alpha, beta, 3)
        assert all(torch.equal(a, b) for a, b in zip(hwc, got))
    unit = rgbd_align.target_intensity_pyramid(dev(render), dev(frame), dev(rendered), dev(filled), 1.0, 0.0, 1)[0].cpu().numpy()
    replaced = filled != rendered
    assert np.array_equal(bits32(unit[replaced]), bits32(ref.grey(frame)[replaced]))
    assert np.array_equal(bits32(unit[~replaced]), bits32(ref.grey(render)[~replaced]))


def test_constants_and_bad_arguments():
    from rtg_slam_amd import _lib, rgbd_align
    lib = _lib.load()
    assert _lib.CONSTANTS["RTGS_RGBD_EXPOSURE_OUT"] == 48 and rgbd_align.OUT8 == 48
    assert lib.rtgs_rgbd_align_exposure_scratch_bytes(60, 80) == 5 * 48 * 8
    assert lib.rtgs_rgbd_align_exposure_scratch_bytes(0, 80) == 0 and lib.rtgs_rgbd_align_exposure_scratch_bytes(65536, 32768) == 0
    s = scene(60, 80)
    d = s["dev"]
    p = lambda t: C.c_void_p(t.data_ptr())
    K, pose = dev(s["K"]), dev(np.eye(4, dtype=np.float32))
    out = torch.full((48,), 7.0, dtype=torch.float64, device=DEV)
    scratch = torch.empty(lib.rtgs_rgbd_align_exposure_scratch_bytes(60, 80) // 8, dtype=torch.float64, device=DEV)

    def call(H=60, W=80, huber=0.05, weight=0.25, alpha=1.0, beta=0.0, null=None):
        ptrs = [p(d[k]) for k in NAMES] + [p(K), p(pose), p(out), p(scratch)]
        if null is not None:
            ptrs[null] = C.c_void_p(0)
        return lib.rtgs_rgbd_align_accumulate_exposure(*ptrs[:6], H, W, ptrs[6], ptrs[7], DIST, COS, weight, huber, alpha, beta,
                                                       ptrs[8], ptrs[9], None)

    assert call(H=0) == -1 and call(W=-3) == -1
    assert call(H=65536, W=32768) == -1                                       # H W = 2^31
    assert call(huber=-0.01) == -1 and call(weight=-1.0) == -1 and call(huber=float("nan")) == -1
    assert call(alpha=float("nan")) == -1 and call(beta=float("nan")) == -1
    for k in range(10):
        assert call(null=k) == -1
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((48,), 7.0, dtype=torch.float64))     # nothing was launched
    colour, depth = torch.zeros(3, 8, 8, device=DEV), torch.ones(8, 8, device=DEV)
    level = torch.full((8, 8), 7.0, device=DEV)
    ptr8 = (C.c_void_p * 1)(level.data_ptr())
    good = [p(colour), p(colour), p(depth), p(depth)]
    for k in range(4):
        bad = list(good)
        bad[k] = C.c_void_p(0)
        assert lib.rtgs_rgbd_target_intensity(*bad, 1.0, 0.0, 8, 8, 1, ptr8, None) == -1
    assert lib.rtgs_rgbd_target_intensity(*good, 1.0, 0.0, 8, 8, 1, None, None) == -1
    assert lib.rtgs_rgbd_target_intensity(*good, 1.0, 0.0, 0, 8, 1, ptr8, None) == -1
    assert lib.rtgs_rgbd_target_intensity(*good, 1.0, 0.0, 8, 8, 0, ptr8, None) == -1
    assert lib.rtgs_rgbd_target_intensity(*good, 1.0, 0.0, 8, 8, 5, ptr8, None) == -1           # 8 >> 4 = 0
    assert lib.rtgs_rgbd_target_intensity(*good, 1.0, 0.0, 8, 8, 1, (C.c_void_p * 1)(None), None) == -1
    torch.cuda.synchronize()
    assert torch.equal(level.cpu(), torch.full((8, 8), 7.0))
    with pytest.raises(ValueError):
        rgbd_align.target_intensity_pyramid(colour, colour, depth, depth, 1.0, 0.0, 5)
    with pytest.raises(ValueError):
        rgbd_align.target_intensity_pyramid(colour[:, :4], colour, depth, depth, 1.0, 0.0, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        rgbd_align.target_intensity_pyramid(colour.cpu(), colour, depth, depth, 1.0, 0.0, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        rgbd_align.accumulate_exposure(*[torch.from_numpy(s[k]) for k in NAMES], K, pose, DIST, COS, 0.25, 0.05, 1.0, 0.0)
    assert call() == 0                                                        # and the same call with nothing wrong runs
    assert lib.rtgs_rgbd_target_intensity(*good, 1.0, 0.0, 8, 8, 1, ptr8, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(level.cpu(), torch.zeros(8, 8))


# ---- the tracker ----

FRAMES, STEP, TILT = 6, 0.02, 10.0
GAINS = ((1.0, 0.0), (1.15, -0.04), (0.9, 0.05), (1.2, -0.06), (0.85, 0.06), (1.1, 0.02))     # (gain, offset) of frame k's colour
HOLE = (slice(20, 32), slice(30, 50))                                        # of the model's render, filled from the frame


def wall_c2w(k):
    """The camera looks at the wall 10 degrees off its normal (a head-on view has one depth, and the normal map drops the
    pixels of the smallest and the largest depth: all of them) and slides 2 cm per frame along the wall."""
    return ref.mrr.rigid((0, 1, 0), TILT, (STEP * k, 0, 0))


def run_tracker(args, gains=None, model=False):
    """tests/test_rgbd_align_gpu.run_tracker, with frame k's colour at gains[k] and, with `model`, the analytic wall seen from
    the ESTIMATED pose standing in for the map's render: unit exposure, a hole in its depth, black where the hole is.
    -> (tracker, what the last update_last_status was given, for the definition's composite)."""
    from rtg_slam_amd import mapping as mp, slam, synth
    K = ref.wall_K()
    cam = synth.CameraSpec(60, 80, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    tracker = slam.Tracker(args, DEV)
    last = None
    for k in range(FRAMES):
        c2w = wall_c2w(k)
        depth, colour, _, _ = ref.wall_view(c2w)
        if gains is not None:
            colour = rer.to_target_exposure(colour, *gains[k])
        frame = mp.Frame(cam, torch.from_numpy(c2w), DEV, uid=k)
        fm = tracker.map_preprocess(frame, dev(depth), dev(colour), k)
        ok = tracker.tracking(frame, fm, pose_gt=c2w, init_pose=c2w if k == 0 else None)
        assert ok, f"frame {k}: ICP's point-to-point loss {tracker.icp_tracker.last_p2ploss}"
        if not model:
            # the sensor depth stands in for the model's render
            tracker.update_last_status(frame, fm["depth_map"].clone(), fm["depth_map"], fm["normal_map_w"].contiguous(), fm["normal_map_w"])
            continue
        est = tracker.pose_es[-1]
        r_depth, r_colour, _, _ = ref.wall_view(est)
        r_depth, r_colour = r_depth.copy(), r_colour.copy()
        # no depth where the frame has none (ICP's point-to-point loss compares the maps pixel by pixel and would count 2 m there)
        r_depth[fm["depth_map"].cpu().numpy().reshape(60, 80) == 0] = 0
        r_depth[HOLE] = 0
        r_colour[(slice(None),) + HOLE] = 0
        r_normal = np.broadcast_to(np.array([0.0, 0.0, -1.0], F32), (60, 80, 3))
        filled = dev(r_depth)[..., None].contiguous()
        exposure = tracker.rgbd_exposure
        tracker.update_last_status(frame, filled, fm["depth_map"], dev(r_normal), fm["normal_map_w"], dev(r_colour).permute(1, 2, 0))
        last = {"render_color": r_colour, "frame_color": colour, "depth_rendered": r_depth, "depth_filled": filled.cpu().numpy()[..., 0],
                "exposure": exposure}
    return tracker, last


def test_tracker_follows_the_wall_through_exposure_changes():
    """The six-frame sliding wall with frame k's colour at GAINS[k] (the gains did not have to be widened).  Final translation
    errors on an MI355X: 0.206 mm with the colour unchanged; with the gains 5.344 mm for rgbd_refine alone, 0.371 mm with
    rgbd_refine_exposure, 0.104 mm with the model target as well (a single-level numpy simulation without ICP in front gave
    4.85 / 0.39 / 0.084 mm).  The model-target run recovers 0.861, 1.099, 0.825, 1.164, 0.899 for the gains' inverses 0.870,
    1.111, 0.833, 1.176, 0.909.  Model against exposure alone is printed, not asserted."""
    from rtg_slam_amd import mapping as mp
    base = dict(use_gt_pose=False, min_depth=0.3, max_depth=8.0, rgbd_refine=True)
    gt = wall_c2w(FRAMES - 1)
    err = lambda t: float(np.linalg.norm(t.pose_es[-1][:3, 3] - gt[:3, 3]))
    assert all(0.8 <= g <= 1.25 and abs(o) <= 0.08 for g, o in GAINS)
    e_on = err(run_tracker(mp.replica_args(**base))[0])
    e_plain = err(run_tracker(mp.replica_args(**base), GAINS)[0])
    t_exp, _ = run_tracker(mp.replica_args(rgbd_refine_exposure=True, **base), GAINS)
    t_model, last = run_tracker(mp.replica_args(rgbd_refine_exposure=True, rgbd_refine_target="model", **base), GAINS, model=True)
    e_exp, e_model = err(t_exp), err(t_model)
    print(f"unchanged colour {1e3 * e_on:.3f} mm; with the gains: plain {1e3 * e_plain:.3f} mm, exposure {1e3 * e_exp:.3f} mm, "
          f"exposure + model target {1e3 * e_model:.3f} mm")
    print("exposure per frame:", [tuple(round(x, 4) for x in r["exposure"]) for r in t_exp.rgbd_reports])
    print("exposure per frame, model target:", [tuple(round(x, 4) for x in r["exposure"]) for r in t_model.rgbd_reports])
    assert e_plain >= 10 * e_on                                               # precondition: the gains do break the plain option
    # the stored target of the next frame is the definition's composite of what the last update_last_status was given
    replaced = last["depth_filled"] != last["depth_rendered"]
    assert replaced[HOLE].all() and not replaced.all()
    assert last["exposure"] == t_model.rgbd_reports[-1]["exposure"] == t_model.rgbd_exposure
    want = rer.target_intensity_pyramid(last["render_color"], last["frame_color"], last["depth_rendered"], last["depth_filled"],
                                        *last["exposure"], 3)
    assert len(t_model.intensity_pyramid_t0) == 3
    for g, w in zip(t_model.intensity_pyramid_t0, want):
        assert np.array_equal(bits32(g.cpu().numpy()), bits32(w))
    assert all(len(r["exposure"]) == 2 for r in t_exp.rgbd_reports) and len(t_exp.rgbd_reports) == FRAMES - 1
    assert e_exp <= 0.25 * e_plain
    assert e_model <= 0.25 * e_plain


def test_defaults_are_untouched(monkeypatch):
    from rtg_slam_amd import _lib, mapping as mp, slam
    lib = _lib.load()
    calls = {n: 0 for n in NEW_ENTRIES}

    def counted(name, fn):
        def wrapper(*a):
            calls[name] += 1
            return fn(*a)
        return wrapper

    for name in NEW_ENTRIES:
        monkeypatch.setattr(lib, name, counted(name, getattr(lib, name)))
    base = dict(use_gt_pose=False, min_depth=0.3, max_depth=8.0, rgbd_refine=True)
    absent = mp.replica_args(**base)
    assert not hasattr(absent, "rgbd_refine_target") and not hasattr(absent, "rgbd_refine_exposure")
    t_absent, _ = run_tracker(absent, GAINS)                                  # update_last_status with five positional arguments
    t_off, _ = run_tracker(mp.replica_args(rgbd_refine_exposure=False, rgbd_refine_target="frame", **base), GAINS)
    assert calls == {n: 0 for n in NEW_ENTRIES}
    assert np.array_equal(np.stack(t_absent.pose_es), np.stack(t_off.pose_es))
    assert not t_off.wants_render_color and t_off.rgbd_exposure == (1.0, 0.0)
    assert all("exposure" not in r for r in t_off.rgbd_reports)
    # the new keys are options of rgbd_refine, and the target is one of two
    off = dict(use_gt_pose=False, min_depth=0.3, max_depth=8.0)
    with pytest.raises(ValueError, match="need rgbd_refine"):
        slam.Tracker(mp.replica_args(rgbd_refine_exposure=True, **off), DEV)
    with pytest.raises(ValueError, match="need rgbd_refine"):
        slam.Tracker(mp.replica_args(rgbd_refine_target="model", **off), DEV)
    with pytest.raises(ValueError, match="'frame' or 'model'"):
        slam.Tracker(mp.replica_args(rgbd_refine_target="map", **base), DEV)
    # with the options on, the new entry points are what runs
    run_tracker(mp.replica_args(rgbd_refine_exposure=True, rgbd_refine_target="model", **base), GAINS, model=True)
    assert calls["rtgs_rgbd_align_accumulate_exposure"] > 0 and calls["rtgs_rgbd_target_intensity"] == FRAMES
