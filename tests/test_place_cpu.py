"""tests/place_reference.py, the definition of the place recognition, on hand-made cases; and, on the CPU, what it is for: a turn in
the box room that comes back to where it began after the trajectory drifted beyond loop_closure_max_trans.

THE TURN (shared with tests/test_place_gpu.py and tests/test_loop_closure_appearance_gpu.py): the turn of
tests/test_loop_closure_gpu.py carried past the full circle - 42 frames at 320 x 240, 10 degrees of yaw a frame about CENTRE;
frames 36 .. 41 are offset by (0.04, -0.02, 0.03) m and 3 degrees of yaw, so that the revisit is not the identical view.
Keyframes [0, 2, 5, ..., 41] (15), min_gap 10.

Measured with the definition (numpy float64, `python -m tests.test_place_cpu` prints it), S = 4, tw = 40:
    pair      true relative pose     score    shift   depth_rel
    (0, 12)   10.00 deg,  0.0 mm     0.9915    +4      0.0546
    (1, 13)    3.00 deg, 53.9 mm     0.9980    -1      0.0172
    (2, 14)    3.00 deg, 53.9 mm     0.9987    -1      0.0158
    (3, 14)   27.00 deg, 53.9 mm     0.9347    +4      0.1075      the nearest other pair; depth_rel just above the 0.1 cut
    (2, 13)   27.00 deg, 53.9 mm     0.8819    +4      0.0625
    (4, 14)   57.00 deg, 53.9 mm     0.8807    +4      0.2681
    every other pair: score <= 0.8015
At 0.9 / 0.1 exactly the first three are candidates.  From appearance_init (off by 1.31, 0.14, 0.14 degrees and 0.0, 53.9,
53.9 mm) tests/rgbd_align_reference.refine lands 0.19, 0.19 and 0.03 mm from the true relative pose with inlier ratios 0.819,
0.945, 0.955, rms 0.3 - 0.4 mm, rank 6, reason done, and every gate of loop_closure.register_pair at loop_args()'s values
passes.  With the drift 12 x UNIT (18 mm and 0.36 degrees a frame, 749 mm at frame 41) find_candidates returns nothing; the pose
graph with the three true edges at weight 2 000 takes the keyframes' rms translation error from 435.6 mm to 24.4 mm."""
import numpy as np
import pytest

from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import pose_graph as pg
from rtg_slam_amd import synth
from rtg_slam_amd.rgbd_align import se3_exp, se3_log
from tests import place_reference as ref
from tests.test_loop_closure_gpu import CAM, CENTRE, UNIT, drifted_poses, kf_rms, loop_args

F32 = np.float32
FRAMES = 42
KEYFRAMES = [0] + list(range(2, FRAMES, 3))                       # 15 keyframes
MIN_GAP = 10
REVISIT_FROM, REVISIT_OFFSET, REVISIT_YAW_DEG = 36, (0.04, -0.02, 0.03), 3.0
DRIFT_SCALE = 12.0
TRUE_PAIRS = {(0, 12): 4, (1, 13): -1, (2, 14): -1}               # pair -> best shift


def turn_poses():
    out = []
    for k in range(FRAMES):
        late = k >= REVISIT_FROM
        T = se3_exp([0.0, np.deg2rad(10.0 * k + (REVISIT_YAW_DEG if late else 0.0)), 0.0, 0.0, 0.0, 0.0])
        T[:3, 3] = np.asarray(CENTRE) + (np.asarray(REVISIT_OFFSET) if late else 0.0)
        out.append(T)
    return out


_turn = {}


def turn_frames():
    """[(depth [1,H,W] or [H,W], colour [3,H,W], true c2w)] of the 42 frames as CPU tensors, rendered once."""
    import torch
    if "frames" not in _turn:
        out = []
        for T in turn_poses():
            p = torch.from_numpy(T)
            d = synth.box_room_depth(CAM, p)
            out.append((d, synth.box_room_color(CAM, p, d), T))
        _turn["frames"] = out
    return _turn["frames"]


def turn_descriptors():
    """The keyframes' descriptors by the definition: three [15, 30, 40] float32 arrays."""
    if "desc" not in _turn:
        fr = turn_frames()
        d = [ref.describe(fr[k][1].numpy(), fr[k][0].numpy(), 40) for k in KEYFRAMES]
        _turn["desc"] = tuple(np.stack([x[i] for x in d]) for i in range(3))
    return _turn["desc"]


def turn_scores():
    if "scores" not in _turn:
        _turn["scores"] = ref.score_pairs(*turn_descriptors(), MIN_GAP, 4)
    return _turn["scores"]


def angle_deg(T):
    return float(np.rad2deg(np.arccos(min(1.0, max(-1.0, (np.trace(T[:3, :3]) - 1.0) / 2.0)))))


# ---- 1. the definition on hand-made cases ----

@pytest.mark.parametrize("H,W,tw,th", [(240, 320, 40, 30), (680, 1200, 40, 23), (45, 67, 8, 5)])
def test_cells_cover_every_pixel_once_and_return_a_cellwise_constant_image(H, W, tw, th):
    assert ref.thumb_height(H, W, tw) == th
    rows, cols = ref.cell_edges(H, th), ref.cell_edges(W, tw)
    count = np.zeros((H, W), dtype=np.int64)
    cell_of = np.zeros((H, W), dtype=np.int64)
    for i in range(th):
        for j in range(tw):
            count[rows[i]:rows[i + 1], cols[j]:cols[j + 1]] += 1
            cell_of[rows[i]:rows[i + 1], cols[j]:cols[j + 1]] = i * tw + j
    assert (count == 1).all()
    sizes = np.bincount(cell_of.reshape(-1))
    assert sizes.size == th * tw and np.ptp(np.diff(rows)) <= 1 and np.ptp(np.diff(cols)) <= 1
    # an image constant per cell, every value a multiple of 1/256 below 4: sums of <= 2^11 of them are exact, so is the mean
    rng = np.random.default_rng(H)
    grey_cell = rng.integers(0, 256, size=th * tw).astype(F32) / F32(256)
    z_cell = rng.integers(64, 1024, size=th * tw).astype(F32) / F32(256)
    g = grey_cell[cell_of]
    color = np.stack([g, g, g])                                   # grey(g, g, g) need not be g: compare with the reference's grey
    from tests.rgbd_align_reference import grey
    want_grey = grey(color)
    inten, dep, val = ref.describe(color, z_cell[cell_of][None], tw)
    assert inten.shape == (th, tw) and inten.dtype == F32
    for i in range(th):
        for j in range(tw):
            cell = want_grey[rows[i]:rows[i + 1], cols[j]:cols[j + 1]]
            assert (cell == cell[0, 0]).all()
            assert inten[i, j] == cell[0, 0]                      # n <= 2^11 equal float32 values: the float64 sum and mean are exact
    assert np.array_equal(dep.reshape(-1), z_cell) and (val == 1).all()


def test_too_large_a_thumbnail_is_refused():
    with pytest.raises(ValueError):
        ref.describe(np.zeros((3, 6, 8), F32), np.zeros((1, 6, 8), F32), 9)


def test_depth_holes_half_valid_and_all_invalid():
    H, W, tw = 12, 16, 4                                          # th 3, cells of 4 x 4
    color = np.random.default_rng(0).random((3, H, W)).astype(F32)
    z = np.full((H, W), 2.0, dtype=F32)
    z[0:4, 0:4] = 0.0                                             # cell (0, 0): no depth
    z[0:2, 4:8] = -1.0                                            # cell (0, 1): exactly half, and negative counts as missing
    z[0:4, 8:12][::2, ::2] = np.nan                               # cell (0, 2): a quarter missing
    inten, dep, val = ref.describe(color, z[None], tw)
    assert dep[0, 0] == 0 and val[0, 0] == 0
    assert dep[0, 1] == 2 and val[0, 1] == F32(0.5)
    assert dep[0, 2] == 2 and val[0, 2] == F32(0.75) and val[1, 1] == 1
    Z = np.zeros((2, 3, 4), dtype=F32)
    I = np.stack([inten, inten])
    sc, sh, rel = ref.pair_scores(I[:1], Z[:1], Z[:1], I[1:], Z[1:], Z[1:], 1)
    assert np.isposinf(rel[0]) and sc[0] == 1 and sh[0] == 0


def test_wave_sum_is_the_stated_tree():
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 200, 1200):
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, size=n)
        lanes = [0.0] * 64
        for p in range(n):
            lanes[p % 64] = lanes[p % 64] + v[p]
        o = 32
        while o:
            lanes = [lanes[l] + lanes[l + o] for l in range(o)]
            o //= 2
        assert ref.wave_sum(v) == lanes[0]


def smooth_thumbnail(seed, th=30, tw=40):
    rng = np.random.default_rng(seed)
    return (rng.random((th, tw)) * 0.5 + 0.25).astype(F32)


@pytest.mark.parametrize("k", [-4, -1, 0, 2, 4])
def test_a_rolled_thumbnail_is_found_at_its_shift(k):
    A = smooth_thumbnail(1)
    B = np.roll(A, k, axis=1)                                     # column x of A sits at column x + k of B
    D = np.ones_like(A)
    sc, sh, rel = ref.pair_scores(A[None], D[None], D[None], B[None], D[None], D[None], 4)
    assert sh[0] == k and abs(float(sc[0]) - 1.0) < 1e-6 and rel[0] == 0


def test_score_is_blind_to_gain_and_offset_and_a_flat_thumbnail_scores_minus_one():
    A, B = smooth_thumbnail(1).astype(np.float64), smooth_thumbnail(2).astype(np.float64)
    for s in (-3, 0, 2):
        base = ref.zncc(A, B, s)
        assert abs(ref.zncc(1.7 * A + 0.3, B, s) - base) < 1e-12 and abs(ref.zncc(A, 0.4 * B + 0.05, s) - base) < 1e-12
        assert abs(ref.zncc(A, A, 0) - 1.0) < 1e-12
    flat = np.full_like(A, 0.5)
    assert ref.zncc(flat, B, 0) == -1 and ref.zncc(A, flat, 1) == -1
    D = np.ones((1, 30, 40), F32)
    sc, sh, rel = ref.pair_scores(flat[None].astype(F32), D, D, B[None].astype(F32), D, D, 4)
    assert sc[0] == -1 and sh[0] == 0                             # all shifts tie at -1: the smallest |s| wins


def test_ties_go_to_the_smaller_shift_then_to_the_negative_one():
    # columns of period 2: every even shift scores 1 exactly, every odd one the same lower value
    A = np.tile(np.array([0.25, 0.75], dtype=F32), (6, 4))        # 6 x 8
    D = np.ones_like(A)
    sc, sh, _ = ref.pair_scores(A[None], D[None], D[None], A[None], D[None], D[None], 3)
    assert sh[0] == 0 and sc[0] == 1
    B = np.roll(A, 1, axis=1)                                     # now -3, -1, +1, +3 tie at 1: -1 wins
    sc, sh, _ = ref.pair_scores(A[None], D[None], D[None], B[None], D[None], D[None], 3)
    assert sh[0] == -1 and sc[0] == 1
    assert ref.shift_order(3) == [0, -1, 1, -2, 2, -3, 3]


def test_sentinels_row_ranges_and_refusals():
    rng = np.random.default_rng(5)
    I, D, V = (rng.random((6, 5, 8)).astype(F32) for _ in range(3))
    sc, sh, rel = ref.score_pairs(I, D, V, 2, 1)
    for b in range(6):
        for a in range(6):
            if a <= b - 2:
                assert -1 <= sc[b, a] <= 1
            else:
                assert sc[b, a] == -2 and sh[b, a] == 0 and np.isposinf(rel[b, a])
    part = ref.score_pairs(I, D, V, 2, 1, rows=(3, 5))
    for whole, p in zip((sc, sh, rel), part):
        assert np.array_equal(p[3:5], whole[3:5])
    assert (part[0][:3] == -2).all() and (part[0][5:] == -2).all()
    for bad in (dict(min_gap=0, S=1), dict(min_gap=1, S=4), dict(min_gap=1, S=-1)):
        with pytest.raises(ValueError):
            ref.score_pairs(I, D, V, bad["min_gap"], bad["S"])


def test_candidates_order_and_limits():
    M = 5
    score = np.full((M, M), -2, F32)
    shift = np.zeros((M, M), np.int32)
    rel = np.full((M, M), np.inf, F32)
    score[4, :4] = [0.95, 0.95, 0.99, 0.5]
    rel[4, :4] = [0.05, 0.02, 0.09, 0.01]
    shift[4, :4] = [1, 2, 3, 4]
    score[3, :3] = [0.95, 0.95, 0.91]
    rel[3, :3] = [0.03, 0.03, 0.2]
    got = ref.find_appearance_candidates(score, shift, rel, 1, 0.9, 0.1, 2)
    assert [(a, b, s) for a, b, _, s, _ in got] == [(0, 3, 0), (1, 3, 0), (2, 4, 3), (1, 4, 2)]
    assert [a for a, *_ in ref.find_appearance_candidates(score, shift, rel, 2, 0.9, 0.1, 5)] == [0, 1, 2, 1, 0]
    from rtg_slam_amd import place_recognition as pr                # the package's copy is the same function
    assert pr.find_appearance_candidates(score, shift, rel, 1, 0.9, 0.1, 2) == got


def test_appearance_init_is_a_yaw():
    from rtg_slam_amd import place_recognition as pr
    T = ref.appearance_init(4, 160.0, 320, 40)
    assert np.allclose(T, se3_exp([0.0, -np.arctan(0.2), 0.0, 0.0, 0.0, 0.0]), atol=1e-15)
    assert abs(np.rad2deg(se3_log(T)[1]) + 11.3099) < 1e-4 and np.array_equal(T[:3, 3], np.zeros(3))
    assert np.array_equal(ref.appearance_init(0, 160.0, 320, 40), np.eye(4))
    assert np.array_equal(pr.appearance_init(-3, 600.0, 1200, 40), ref.appearance_init(-3, 600.0, 1200, 40))


# ---- 2. the turn ----

def test_the_turn_yields_its_three_revisits():
    score, shift, rel = turn_scores()
    truth = [turn_poses()[k] for k in KEYFRAMES]
    got = ref.find_appearance_candidates(score, shift, rel, MIN_GAP)
    print("candidates:", [(a, b, round(sc, 4), sh, round(dr, 4)) for a, b, sc, sh, dr in got])
    found = {(a, b): sh for a, b, _, sh, _ in got}
    for pair, sh in TRUE_PAIRS.items():
        assert found.get(pair) == sh, (pair, found)
    for a, b, *_ in got:
        assert angle_deg(pg.inverse(truth[a]) @ truth[b]) <= 35.0, (a, b)


# ---- 3. registration from the appearance guess ----

class NumpyRefiner:
    """tests/rgbd_align_reference.refine behind the interface register_pair uses."""
    exposure = False

    def refine(self, init, v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, K, downscales):
        from tests import rgbd_align_reference as rar
        Z, rep = rar.refine(init, v_src, n_src, i_src, v_tgt, n_tgt, i_tgt, np.asarray(K), list(downscales), distance_threshold=0.1,
                            cos_threshold=float(np.cos(np.deg2rad(20.0))))
        rep["device_s"] = 0.0
        return Z, rep


def keyframe_pyramids(k):
    import torch
    from oracle import icp_oracle as io
    from tests import rgbd_align_reference as rar
    key = ("pyr", k)
    if key not in _turn:
        K = torch.tensor([[CAM.fx, 0, CAM.cx], [0, CAM.fy, CAM.cy], [0, 0, 1]], dtype=torch.float32)
        d, c, _ = turn_frames()[KEYFRAMES[k]]
        vp = io.vertex_pyramid(d, K, 3)
        _turn[key] = {"vertex": [x.numpy() for x in vp], "normal": [x.numpy() for x in io.normal_pyramid(vp)],
                      "intensity": rar.intensity_pyramid(c.numpy(), 3)}
    return _turn[key]


def register_from_appearance(pair, shift, cfg):
    a, b = pair
    K = np.array([[CAM.fx, 0, CAM.cx], [0, CAM.fy, CAM.cy], [0, 0, 1]], dtype=np.float32)
    init = ref.appearance_init(shift, CAM.fx, CAM.W, 40)
    return lc.register_pair(NumpyRefiner(), keyframe_pyramids(b), keyframe_pyramids(a), init, K, [0.25, 0.5, 1.0], cfg), init


@pytest.mark.parametrize("pair", sorted(TRUE_PAIRS))
def test_the_revisits_register_from_the_appearance_guess(pair):
    truth = [turn_poses()[k] for k in KEYFRAMES]
    want = pg.inverse(truth[pair[0]]) @ truth[pair[1]]
    cfg = lc.LoopCloser(loop_args()).cfg
    r, init = register_from_appearance(pair, TRUE_PAIRS[pair], cfg)
    off = pg.inverse(want) @ init
    err = float(np.linalg.norm(r["Z"][:3, 3] - want[:3, 3]))
    print(f"{pair}: guess off by {angle_deg(off):.2f} degrees / {1e3 * np.linalg.norm(init[:3, 3] - want[:3, 3]):.1f} mm -> "
          f"{1e3 * err:.2f} mm from the truth, {r['reason']}, inlier ratio {r['inlier_ratio']:.3f}, rms "
          f"{1e3 * r['rms_geometric_after']:.2f} mm, rank {r['rank_min']}, correction {1e3 * r['correction_trans']:.1f} mm / "
          f"{r['correction_rot_deg']:.2f} degrees")
    assert r["accepted"], r["reason"]
    assert err < 1e-3 and angle_deg(pg.inverse(want) @ r["Z"]) < 0.1


# ---- 4. the drift hides the loop from the poses; the three edges close it ----

def test_the_drifted_poses_hide_the_loop_and_the_three_edges_close_it():
    truth = turn_poses()
    drifted = drifted_poses(truth, DRIFT_SCALE * UNIT)
    kf_true, kf_old = [truth[k] for k in KEYFRAMES], [drifted[k] for k in KEYFRAMES]
    cfg = lc.LoopCloser(loop_args()).cfg
    assert cfg.max_trans == 0.5 and cfg.max_rot_deg == 35.0 and cfg.min_gap == MIN_GAP
    assert lc.find_candidates(kf_old, KEYFRAMES, cfg.min_gap, cfg.max_trans, cfg.max_rot_deg, cfg.max_per_keyframe) == []
    edges = [(k - 1, k, pg.inverse(kf_old[k - 1]) @ kf_old[k], 1.0, 1.0) for k in range(1, len(KEYFRAMES))]
    edges += [(a, b, pg.inverse(kf_true[a]) @ kf_true[b], 2000.0, 2000.0, True) for a, b in TRUE_PAIRS]
    new, _ = pg.optimize(kf_old, edges, fixed=0, huber=None)
    before, after = kf_rms(kf_old, kf_true), kf_rms(new, kf_true)
    print(f"drift at frame 41: {1e3 * np.linalg.norm(drifted[41][:3, 3] - truth[41][:3, 3]):.0f} mm; keyframe rms "
          f"{1e3 * before:.1f} -> {1e3 * after:.1f} mm")
    assert after < 0.5 * before


def test_the_new_keys_default_to_pose_and_are_validated():
    closer = lc.LoopCloser(loop_args())
    assert vars(closer.place) == dict(candidates="pose", thumb_width=40, max_shift=4, min_score=0.9, max_depth_rel=0.1)
    assert not any(k in vars(closer.cfg) for k in vars(closer.place))        # the report's options stay what they were
    for over in (dict(loop_closure_candidates="orb"), dict(loop_closure_thumb_width=0), dict(loop_closure_max_shift=20),
                 dict(loop_closure_min_score=1.01), dict(loop_closure_max_depth_rel=-1e-3)):
        with pytest.raises(ValueError):
            lc.LoopCloser(loop_args(**over))


def print_figures():
    score, shift, rel = turn_scores()
    truth = [turn_poses()[k] for k in KEYFRAMES]
    rows = []
    for b in range(len(KEYFRAMES)):
        for a in range(0, b - MIN_GAP + 1):
            T = pg.inverse(truth[a]) @ truth[b]
            rows.append((float(score[b, a]), a, b, int(shift[b, a]), float(rel[b, a]), angle_deg(T), 1e3 * np.linalg.norm(T[:3, 3])))
    for sc, a, b, sh, dr, ang, mm in sorted(rows, reverse=True):
        print(f"({a:2d}, {b:2d})  {ang:6.2f} deg {mm:6.1f} mm   score {sc:.4f}  shift {sh:+d}  depth_rel {dr:.4f}")
    cfg = lc.LoopCloser(loop_args()).cfg
    for pair, sh in TRUE_PAIRS.items():
        test_the_revisits_register_from_the_appearance_guess(pair)
    test_the_drifted_poses_hide_the_loop_and_the_three_edges_close_it()


if __name__ == "__main__":
    print_figures()
