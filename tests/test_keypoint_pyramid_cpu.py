"""tests/keypoint_pyramid_reference.py, the definition of the keypoints over an image pyramid and of the keypoint votes, on hand-made
cases; and, on the CPU, what it is for: a revisit of the textured box room seen from further away, which the single-scale
keypoints and the thumbnails both miss.

THE FAR PAIRS (`python -m tests.test_keypoint_pyramid_cpu` prints them): the textured room of tests/test_keypoints_cpu.py, view B
is view A moved straight back along its own optical axis.  Matches are the filtered mutual matches, inliers those of
keypoint_reference.ransac_rigid, the gate is min_inliers = 8, which stays what it is.
    start yaw   moved back   centre depth A -> B (ratio)   1 level: matches / inliers   3 levels: matches / inliers, pose error   5 levels
        0         0.4 m       2.77 -> 3.17 (1.14)               43 / 37                    68 / 60,  3.2 mm                         76 / 66
        0         0.8 m       2.77 -> 3.57 (1.29)               18 /  7                    45 / 38,  2.8 mm                         54 / 45
        0         1.2 m       2.77 -> 3.96 (1.43)               13 /  3                    52 / 41, 28.5 mm                         59 / 45
       50         0.8 m       3.05 -> 3.85 (1.26)               22 /  9                    57 / 42, 20.9 mm                         63 / 46
       50         1.2 m       3.05 -> 4.25 (1.39)               15 /  1                    45 / 26, 12.9 mm                         54 / 30
    right pairs 1.2 m apart at 3 levels, from yaw 0, 50, 120: 52 / 41, 45 / 26, 49 / 36.
    wrong pairs at 3 levels (from yaw 0): the wall 90 degrees to the right 15 matches / 1 inlier, the opposite wall 21 / 1; the
    same two walls seen from 1.2 m further back 28 / 1 and 29 / 1.
The conditions the tests hold the definition to: at 1 level every pair at a depth ratio of 1.39 or more ends below 8 inliers; at 3
levels every pair reaches 8 and its pose lies inside register_pair's correction gate; the wrong pairs stay at or below 2.

THE FAR TURN (shared with the GPU tests of the keypoint search and of the far relocalisation): the turn of
tests/test_keypoints_cpu.py with its revisit frames 36 .. 41 moved back along each frame's own optical axis by FAR_BACK = 1.2 m
(no yaw, no roll, nothing sideways).  With the definitions, S = 4, tw = 40, the revisit pairs (1, 13) and (2, 14):
    pair      score    depth_rel   1 level: matches / inliers   3 levels: matches / inliers   3-level pose off by
    (1, 13)   0.7795    0.1878            25 / 1                        64 / 35                20.2 mm, 0.26 deg
    (2, 14)   0.7718    0.2054            15 / 1                        45 / 26                12.9 mm, 0.17 deg
so the thumbnails refuse both (score below 0.9, depth_rel above 0.1) and one level ends far below the gate.  From the 3-level pose
tests/rgbd_align_reference.refine lands 2.52 and 2.34 mm from the truth and every gate of register_pair passes: inlier ratios
0.386 and 0.370 against min_inlier_ratio 0.3 (about half of the far view's pixels fall inside the near view), corrections 22.5
and 11.8 mm.  The offset was chosen on the CPU as a condition - depth_rel > 0.1, one level below 8, three levels at least 8,
register_pair accepts - and 1.2 m, the first tried, meets all four."""
import numpy as np
import pytest

from rtg_slam_amd import keypoints as kp
from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import pose_graph as pg
from tests import keypoint_pyramid_reference as pyr
from tests import keypoint_reference as ref
from tests.test_keypoints_cpu import K_CAM, image_of, random_desc, textured_view, view_pose
from tests.test_loop_closure_gpu import CAM, loop_args
from tests.test_place_cpu import FRAMES, KEYFRAMES, REVISIT_FROM, NumpyRefiner, angle_deg

F32 = np.float32
FAR_BACK = 1.2                                                     # metres the far turn's revisit frames are moved back
FAR_PAIRS = ((1, 13), (2, 14))                                     # its keyframe pairs that see one place from two distances
FAR_TABLE = ((0.0, 0.4), (0.0, 0.8), (0.0, 1.2), (50.0, 0.8), (50.0, 1.2))      # (start yaw in degrees, metres moved back)
_cache = {}


def moved_back(T, metres):
    """The c2w pose T moved back along its own optical axis (the camera's z)."""
    out = np.array(T, dtype=np.float64)
    out[:3, 3] -= float(metres) * out[:3, 2]
    return out


def features_of(T, levels):
    """The definition's features of the textured view at T over `levels` levels, with "xyz"; computed once per pose and count."""
    key = ("feat", np.asarray(T).tobytes(), int(levels))
    if key not in _cache:
        d, c = textured_view(T)
        f = pyr.detect_and_describe(c.numpy(), d.numpy().reshape(CAM.H, CAM.W), levels=levels)
        f["xyz"] = pyr.backproject(f, K_CAM)
        _cache[key] = f
    return _cache[key]


def reference_pose(Ta, Tb, levels):
    """-> (matches, inliers, T or None, the true T_a^-1 T_b) by the definitions alone."""
    fa, fb = features_of(Ta, levels), features_of(Tb, levels)
    m = ref.filter_matches(ref.match(fb["desc"], fa["desc"]), ref.match(fa["desc"], fb["desc"]))
    want = pg.inverse(Ta) @ Tb
    fit = ref.ransac_rigid(fa["xyz"][[j for _, j, _ in m]], fb["xyz"][[i for i, _, _ in m]]) if len(m) >= 3 else None
    if fit is None:
        return len(m), 0, None, want
    return len(m), int(fit[1].sum()), fit[0], want


def far_turn_poses():
    return [moved_back(view_pose(10.0 * k), FAR_BACK if k >= REVISIT_FROM else 0.0) for k in range(FRAMES)]


def far_turn_frames():
    """[(depth, colour, true c2w)] of the 42 frames of the far turn as CPU tensors, rendered once."""
    if "turn" not in _cache:
        _cache["turn"] = [textured_view(T) + (T,) for T in far_turn_poses()]
    return _cache["turn"]


def centre_depth(T):
    return float(textured_view(T)[0].numpy().reshape(CAM.H, CAM.W)[CAM.H // 2, CAM.W // 2])


# ---- 1. the reductions on hand-made images ----

def test_a_constant_image_stays_constant_on_every_level():
    g = np.full((35, 50), 137, np.uint8)
    for l, (p, _) in enumerate(pyr.pyramid(image_of(g), np.ones(g.shape, F32), pyr.level_table(35, 50, 5))):
        assert p.dtype == np.uint8 and (p == 137).all(), l
    assert (pyr.reduce2(np.full((7, 9), 255, np.uint8)) == 255).all() and (pyr.reduce32(np.full((7, 9), 255, np.uint8)) == 255).all()
    assert (pyr.reduce32(np.zeros((6, 6), np.uint8)) == 0).all()


def test_stripes_have_their_exact_integer_results():
    # 3-periodic columns 0, 90, 255: output 2k = (2 * 0 + 90) * 3 / 9 = 30, output 2k + 1 = (90 + 2 * 255) * 3 / 9 = 200
    g = np.tile(np.array([0, 90, 255], np.uint8), (6, 4))
    assert g.shape == (6, 12)
    r = pyr.reduce32(g)
    assert r.shape == (4, 8) and (r[:, 0::2] == 30).all() and (r[:, 1::2] == 200).all()
    assert np.array_equal(pyr.reduce32(g.T.copy()), r.T)
    # the rounding: (2 * 10 + 11) * 3 = 93 -> (93 + 4) // 9 = 10;  (11 + 2 * 13) * 3 = 111 -> 115 // 9 = 12
    g = np.tile(np.array([10, 11, 13], np.uint8), (3, 2))
    assert pyr.reduce32(g).tolist() == [[10, 12, 10, 12]] * 2
    # 2-periodic columns 10, 13: every block sums to 46 -> (46 + 2) >> 2 = 12; rows 10, 13 the same
    g = np.tile(np.array([10, 13], np.uint8), (4, 5))
    assert (pyr.reduce2(g) == 12).all() and pyr.reduce2(g).shape == (2, 5) and (pyr.reduce2(g.T.copy()) == 12).all()
    # one bright pixel in a 2 x 2 block: (255 + 2) >> 2 = 64; in a 3 x 3 block, the corner weights 4, 2, 2, 1
    g = np.zeros((4, 4), np.uint8)
    g[0, 0] = 255
    assert pyr.reduce2(g).tolist() == [[64, 0], [0, 0]]
    g = np.zeros((3, 3), np.uint8)
    g[0, 0] = 255
    assert pyr.reduce32(g).tolist() == [[(4 * 255 + 4) // 9, 0], [0, 0]]
    g[0, 0], g[1, 1] = 0, 255                                       # the middle pixel has weight 1 in each of the four outputs
    assert pyr.reduce32(g).tolist() == [[28, 28], [28, 28]]


@pytest.mark.parametrize("H,W", [(35, 50), (33, 47)])
def test_odd_sizes_drop_the_trailing_rows_and_columns(H, W):
    rng = np.random.default_rng(H)
    g = rng.integers(0, 256, size=(H, W)).astype(np.uint8)
    sizes = pyr.level_sizes(H, W, 5)
    assert sizes == [(H, W), (2 * (H // 3), 2 * (W // 3)), (H // 2, W // 2), (H // 3, W // 3), (H // 4, W // 4)]
    r2, r32 = pyr.reduce2(g), pyr.reduce32(g)
    assert r2.shape == sizes[2] and r32.shape == sizes[1]
    assert np.array_equal(r2, pyr.reduce2(g[:2 * (H // 2), :2 * (W // 2)]))           # what was dropped did not count
    assert np.array_equal(r32, pyr.reduce32(g[:3 * (H // 3), :3 * (W // 3)]))
    # against the rule written out pixel by pixel
    y, x = sizes[2][0] - 1, sizes[2][1] - 1
    assert r2[y, x] == (int(g[2 * y, 2 * x]) + int(g[2 * y, 2 * x + 1]) + int(g[2 * y + 1, 2 * x]) + int(g[2 * y + 1, 2 * x + 1]) + 2) >> 2
    for y, x in ((0, 0), (1, 0), (0, 1), (sizes[1][0] - 1, sizes[1][1] - 1), (5, 8)):
        wy = {3 * (y // 2) + (y & 1): 2 - (y & 1), 3 * (y // 2) + (y & 1) + 1: 1 + (y & 1)}
        wx = {3 * (x // 2) + (x & 1): 2 - (x & 1), 3 * (x // 2) + (x & 1) + 1: 1 + (x & 1)}
        assert r32[y, x] == (sum(a * b * int(g[yy, xx]) for yy, a in wy.items() for xx, b in wx.items()) + 4) // 9
    table = pyr.level_table(H, W, 5)
    levels = pyr.pyramid(image_of(g), np.arange(H * W, dtype=F32).reshape(H, W), table)
    assert [p[0].shape for p in levels] == sizes and np.array_equal(levels[3][0], pyr.reduce2(r32)) and np.array_equal(levels[4][0], pyr.reduce2(r2))
    # the level depth is level 0's under the pixel's centre: columns 0, 2, 3, 5 .. at 3/2; 1, 3 .. at 2; 1, 4 .. at 3; 2, 6 .. at 4
    for l, first in ((1, [0, 2, 3, 5]), (2, [1, 3, 5, 7]), (3, [1, 4, 7, 10]), (4, [2, 6, 10, 14])):
        assert np.array_equal(levels[l][1][:4, :4], (np.asarray(first)[:, None] * W + np.asarray(first)[None, :]).astype(F32))
        assert levels[l][1].max() < H * W
    assert np.array_equal(levels[0][1], np.arange(H * W, dtype=F32).reshape(H, W))


def test_a_level_that_cannot_hold_a_cell_is_dropped_with_all_after_it():
    t = pyr.level_table(240, 320, 5, 16)
    assert t[:, 1:3].tolist() == [[240, 320], [160, 212], [120, 160], [80, 106], [60, 80]] and t[:, 3:].tolist() == [list(s) for s in pyr.SCALES]
    assert t[:, 0].tolist() == [0, 76800, 76800 + 160 * 212, 76800 + 160 * 212 + 120 * 160, 76800 + 160 * 212 + 120 * 160 + 80 * 106]
    t = pyr.level_table(120, 160, 5, 16)                            # level 3 would be 40 x 53: 40 < 32 + 16
    assert t[:, 1:3].tolist() == [[120, 160], [80, 106], [60, 80]]
    assert len(pyr.level_table(120, 160, 5, 8)) == 4                # 40 x 53 holds a cell of 8, level 4's 30 x 40 does not
    assert len(pyr.level_table(35, 50, 5, 16)) == 1 and len(pyr.level_table(35, 50, 5)) == 5       # level 0 is always there
    assert len(pyr.level_table(71, 200, 3, 16)) == 1                # level 1 is 46 rows: dropped, and level 2 with it
    for H, W in ((240, 320), (120, 160), (35, 50), (33, 47), (71, 200), (680, 1200)):
        for L in range(1, 6):
            for c in (8, 16, 32):
                assert np.array_equal(kp.level_table(H, W, L, c), pyr.level_table(H, W, L, c)), (H, W, L, c)
    with pytest.raises(ValueError):
        pyr.level_table(240, 320, 6)
    color, depth = image_of(np.random.default_rng(2).integers(0, 256, size=(120, 160)).astype(np.uint8)), np.ones((120, 160), F32)
    assert pyr.detect_and_describe(color, depth, levels=5)["levels_used"] == 3


def test_one_level_is_the_single_scale_definition_array_for_array():
    d, c = textured_view(view_pose(20.0))
    z = d.numpy().reshape(CAM.H, CAM.W)
    one, want = pyr.detect_and_describe(c.numpy(), z, levels=1), ref.detect_and_describe(c.numpy(), z)
    for k in ("slots", "slot_desc", "x", "y", "score", "bin", "desc"):
        assert one[k].dtype == want[k].dtype and np.array_equal(one[k], want[k]), k
    assert np.array_equal(one["g8"][0], want["g8"]) and np.array_equal(one["box5"][0], want["box5"]) and one["levels_used"] == 1
    assert (one["level"] == 0).all() and np.array_equal(one["x0"], want["x"].astype(np.float64)) and np.array_equal(one["y0"], want["y"])
    assert np.array_equal(pyr.backproject(one, K_CAM), ref.backproject(want["x"], want["y"], z, K_CAM))


def test_the_levels_follow_each_other_and_x0_is_the_pixel_centre():
    d, c = textured_view(view_pose(20.0))
    f = pyr.detect_and_describe(c.numpy(), d.numpy().reshape(CAM.H, CAM.W), levels=3)
    assert f["levels_used"] == 3 and (np.diff(f["level"]) >= 0).all() and set(f["level"].tolist()) == {0, 1, 2}
    cells = [(-(-h // 16)) * (-(-w // 16)) for _, h, w, _, _ in f["table"].tolist()]
    assert len(f["slots"]) == sum(cells) and np.array_equal(f["slot_level"], np.repeat([0, 1, 2], cells))
    n0 = int((f["level"] == 0).sum())
    one = pyr.detect_and_describe(c.numpy(), d.numpy().reshape(CAM.H, CAM.W), levels=1)
    assert np.array_equal(f["desc"][:n0], one["desc"]) and np.array_equal(f["x"][:n0], one["x"])      # level 0 is untouched by the others
    for l, s in ((1, 1.5), (2, 2.0)):
        m = f["level"] == l
        assert m.sum() > 10 and np.array_equal(f["x0"][m], (f["x"][m] + 0.5) * s - 0.5) and np.array_equal(f["y0"][m], (f["y"][m] + 0.5) * s - 0.5)
        h, w = f["table"][l, 1:3]
        assert f["x"][m].min() >= 16 and f["x"][m].max() < w - 16 and f["y"][m].min() >= 16 and f["y"][m].max() < h - 16
    xyz = pyr.backproject(f, K_CAM)
    k = int(np.nonzero(f["level"] == 2)[0][0])
    z = d.numpy().reshape(CAM.H, CAM.W)[2 * f["y"][k] + 1, 2 * f["x"][k] + 1]
    assert xyz[k, 2] == float(z) and xyz[k, 0] == (f["x0"][k] - K_CAM[0, 2]) / K_CAM[0, 0] * float(z)


# ---- 2. the far pairs ----

@pytest.mark.parametrize("yaw,back", FAR_TABLE)
def test_far_pairs_need_the_pyramid(yaw, back):
    cfg = lc.LoopCloser(loop_args())
    A = view_pose(yaw)
    B = moved_back(A, back)
    ratio = centre_depth(B) / centre_depth(A)
    n1, i1, _, want = reference_pose(A, B, 1)
    n3, i3, T3, _ = reference_pose(A, B, 3)
    print(f"yaw {yaw:g}, {back} m back, depth ratio {ratio:.2f}: 1 level {n1} / {i1}, 3 levels {n3} / {i3}")
    assert cfg.keypoints.cfg.min_inliers == 8
    if ratio >= 1.39:
        assert i1 < 8
    assert i3 >= 8
    err, ang = float(np.linalg.norm(T3[:3, 3] - want[:3, 3])), angle_deg(pg.inverse(want) @ T3)
    assert err <= cfg.cfg.max_correction_trans and ang <= cfg.cfg.max_correction_rot_deg


@pytest.mark.parametrize("turn,back", [(90.0, 0.0), (180.0, 0.0), (90.0, 1.2), (180.0, 1.2)])
def test_wrong_walls_stay_at_or_below_two_inliers_at_three_levels(turn, back):
    n, inl, _, _ = reference_pose(view_pose(0.0), moved_back(view_pose(turn), back), 3)
    print(f"the wall {turn:g} degrees on, {back} m back: {n} matches, {inl} inliers")
    assert n >= 3 and inl <= 2


# ---- 3. the votes and the shortlist ----

def test_votes_are_the_length_of_the_filter():
    q, r = random_desc(300, 4), random_desc(257, 5)                 # more than 256 references: the match kernel's second tile
    r[::3] = q[:len(r[::3])] ^ np.uint32(1)                         # near hits
    m_ba, m_ab = ref.match(q, r), ref.match(r, q)
    n = pyr.votes(m_ba, m_ab)
    assert n == len(ref.filter_matches(m_ba, m_ab)) == len(kp.filter_matches(m_ba, m_ab)) == 86
    assert pyr.votes(m_ba, m_ab, max_hamming=0) == 0 and pyr.votes(m_ba, m_ab, 256, 1.0) >= n
    empty = np.empty((0, 3), np.int32)
    assert pyr.votes(empty, empty) == 0 and pyr.votes(ref.match(q, r[:0]), empty) == 0 and pyr.votes(empty, ref.match(r, q[:0])) == 0
    same = np.repeat(q[:1], 5, axis=0)                              # ties: every best is index 0 at distance 0, second 0 as well
    assert pyr.votes(ref.match(same, same), ref.match(same, same)) == 1 and pyr.votes(ref.match(same, same), ref.match(same, same), 64, 0.0) == 1
    two = np.concatenate([q[:1], q[:1] ^ np.uint32(1)])             # 0 <= 0.8 x 1 passes; 1 <= 0.8 x 1 does not
    assert pyr.votes(ref.match(two, two[:1]), ref.match(two[:1], two)) == 1


def test_the_shortlist_takes_the_most_votes_and_ties_go_to_the_lower_index():
    for f in (pyr.top_k, kp.shortlist):
        assert f([9, 30, 8, 30, 12, 7], 3, 8) == [1, 3, 4]
        assert f([9, 30, 8, 30, 12, 7], 2, 8) == [1, 3] and f([9, 30, 8, 30, 12, 7], 9, 8) == [1, 3, 4, 0, 2]
        assert f([7, 7, 7], 3, 8) == [] and f([], 3, 8) == [] and f([8, 8, 8], 2, 8) == [0, 1]
        assert f(np.array([5, 9, 9], np.int32), 1, 3) == [1]


# ---- 4. the far turn ----

def far_pyramids(k):
    import torch
    from oracle import icp_oracle as io
    from tests import rgbd_align_reference as rar
    key = ("pyr", k)
    if key not in _cache:
        d, c, _ = far_turn_frames()[KEYFRAMES[k]]
        vp = io.vertex_pyramid(d, torch.tensor(K_CAM, dtype=torch.float32), 3)
        _cache[key] = {"vertex": [x.numpy() for x in vp], "normal": [x.numpy() for x in io.normal_pyramid(vp)],
                       "intensity": rar.intensity_pyramid(c.numpy(), 3)}
    return _cache[key]


def far_pair_figures(pair):
    """The thumbnails' verdict and the keypoint poses at one and at three levels of a keyframe pair of the far turn."""
    from tests import place_reference as pref
    a, b = pair
    fr = far_turn_frames()
    A, B = (pref.describe(fr[KEYFRAMES[k]][1].numpy(), fr[KEYFRAMES[k]][0].numpy(), 40) for k in (a, b))
    sc, sh, rel = pref.pair_scores(A[0][None], A[1][None], A[2][None], B[0][None], B[1][None], B[2][None], 4)
    Ta, Tb = fr[KEYFRAMES[a]][2], fr[KEYFRAMES[b]][2]
    return float(sc[0]), float(rel[0]), reference_pose(Ta, Tb, 1), reference_pose(Ta, Tb, 3)


@pytest.mark.parametrize("pair", FAR_PAIRS)
def test_the_far_revisit_is_refused_by_the_thumbnails_missed_at_one_level_and_registers_from_three(pair):
    cfg = lc.LoopCloser(loop_args()).cfg
    score, rel, (n1, i1, _, _), (n3, i3, T3, want) = far_pair_figures(pair)
    print(f"{pair}: score {score:.4f}, depth_rel {rel:.4f}; 1 level {n1} matches / {i1} inliers; 3 levels {n3} / {i3}")
    assert rel > 0.1                                                # 1. the thumbnails refuse the pair
    assert i1 < 8                                                   # 2. one level ends below the gate
    assert i3 >= 8                                                  # 3. three levels pass it
    r = lc.register_pair(NumpyRefiner(), far_pyramids(pair[1]), far_pyramids(pair[0]), T3, K_CAM.astype(F32), [0.25, 0.5, 1.0], cfg)
    err = float(np.linalg.norm(r["Z"][:3, 3] - want[:3, 3]))
    print(f"{pair} from the 3-level pose ({1e3 * np.linalg.norm(T3[:3, 3] - want[:3, 3]):.1f} mm / {angle_deg(pg.inverse(want) @ T3):.2f} degrees off): "
          f"{r['reason']}, {1e3 * err:.2f} mm from the truth, inlier ratio {r['inlier_ratio']:.3f}, correction {1e3 * r['correction_trans']:.1f} mm")
    assert r["accepted"], r["reason"]                               # 4. register_pair accepts from the three-level guess
    assert err < 5e-3


# ---- 5. the keys and the flags ----

def test_the_new_keys_are_absent_by_default_and_validated():
    from rtg_slam_amd import relocalisation as rl
    closer = lc.LoopCloser(loop_args())
    assert "levels" not in vars(closer.keypoints.cfg) and not hasattr(closer.keypoints, "shortlist") and closer.place.candidates == "pose"
    assert not any("levels" in k or "shortlist" in k for k in lc.DEFAULTS) and "levels" not in kp.DEFAULTS
    on = lc.LoopCloser(loop_args(loop_closure_candidates="keypoints", loop_closure_keypoint_levels=3))
    assert (on.keypoints.cfg.levels, on.keypoints.init, on.keypoints.ransac, on.keypoints.shortlist) == (3, "keypoints_strict", "device", 3)
    lc.LoopCloser(loop_args(loop_closure_candidates="both", loop_closure_appearance_init="keypoints", loop_closure_keypoint_levels=5))
    lc.LoopCloser(loop_args(loop_closure_candidates="keypoints", loop_closure_appearance_init="keypoints_strict", loop_closure_keypoint_ransac="device",
                            loop_closure_keypoint_shortlist=1))
    for over in (dict(loop_closure_keypoint_levels=0), dict(loop_closure_keypoint_levels=6), dict(loop_closure_keypoint_levels=1.5),
                 dict(loop_closure_keypoint_levels=True), dict(loop_closure_candidates="keypoints", loop_closure_appearance_init="keypoints"),
                 dict(loop_closure_candidates="keypoints", loop_closure_appearance_init="yaw"),
                 dict(loop_closure_candidates="keypoints", loop_closure_keypoint_ransac="host"),
                 dict(loop_closure_candidates="keypoints", loop_closure_keypoint_shortlist=0), dict(loop_closure_keypoint_shortlist=3),
                 dict(loop_closure_candidates="keypoints", loop_closure_keypoint_ransac_iters=70000)):
        with pytest.raises(ValueError):
            lc.LoopCloser(loop_args(**over))
    r = rl.Relocaliser(loop_args(use_gt_pose=False, relocalise=True))
    assert r.search == "thumbnails" and "search" not in r.options() and "keypoint_levels" not in r.options() and set(r.seconds) == set(rl.STAGES)
    r = rl.Relocaliser(loop_args(use_gt_pose=False, relocalise=True, relocalise_search="keypoints", relocalise_keypoint_levels=3))
    assert r.options()["search"] == "keypoints" and r.options()["keypoint_levels"] == 3 and r.kc.levels == 3 and set(r.seconds) == set(rl.KEYPOINT_STAGES)
    assert rl.Relocaliser(loop_args(use_gt_pose=False, loop_closure_keypoint_levels=2, relocalise_keypoint_levels=4)).kc.levels == 4
    assert rl.Relocaliser(loop_args(use_gt_pose=False, loop_closure_keypoint_levels=2)).kc.levels == 2
    for over in (dict(relocalise_search="orb"), dict(relocalise_keypoint_levels=0), dict(relocalise_keypoint_levels=6)):
        with pytest.raises(ValueError):
            rl.Relocaliser(loop_args(**dict(dict(use_gt_pose=False), **over)))
    with pytest.raises(ValueError, match="relocalise_keypoint_levels"):
        rl.Relocaliser(loop_args(use_gt_pose=False, relocalise_keypoint_levels=9))


def test_the_cli_flags_set_the_keys_only_when_given():
    from types import SimpleNamespace
    from rtg_slam_amd import __main__ as cli
    parse = lambda argv: cli.build_parser().parse_args(["slam", "--config", "x.yaml"] + argv)
    args = SimpleNamespace()
    assert cli._apply_loop_closure(args, parse(["--loop-closure", "--loop-closure-candidates", "keypoints", "--loop-closure-keypoint-levels", "3",
                                                "--loop-closure-keypoint-shortlist", "4"])) is None
    assert vars(args) == dict(loop_closure=True, loop_closure_candidates="keypoints", loop_closure_keypoint_levels=3, loop_closure_keypoint_shortlist=4)
    args = SimpleNamespace()
    assert cli._apply_loop_closure(args, parse(["--loop-closure"])) is None and vars(args) == dict(loop_closure=True)      # config.yaml: nothing new
    said = cli._apply_loop_closure(SimpleNamespace(), parse(["--loop-closure-keypoint-levels", "3"]))
    assert said is not None and "needs --loop-closure" in said
    said = cli._apply_loop_closure(SimpleNamespace(), parse(["--loop-closure", "--loop-closure-keypoint-levels", "7"]))
    assert said is not None and "loop_closure_keypoint_levels" in said
    said = cli._apply_loop_closure(SimpleNamespace(), parse(["--loop-closure", "--loop-closure-candidates", "keypoints", "--loop-closure-appearance-init", "yaw"]))
    assert said is not None and "keypoints_strict" in said
    said = cli._apply_loop_closure(SimpleNamespace(), parse(["--loop-closure", "--loop-closure-keypoint-shortlist", "2"]))
    assert said is not None and "loop_closure_candidates keypoints" in said
    base = lambda: SimpleNamespace(**vars(loop_args(use_gt_pose=False)))
    args = base()
    before = dict(vars(args))
    assert cli._apply_relocalise(args, parse(["--relocalise", "--relocalise-search", "keypoints", "--relocalise-keypoint-levels", "3"])) is None
    assert {k: v for k, v in vars(args).items() if k not in before} == dict(relocalise=True, relocalise_search="keypoints", relocalise_keypoint_levels=3)
    said = cli._apply_relocalise(base(), parse(["--relocalise-search", "keypoints"]))
    assert said is not None and "needs --relocalise" in said
    said = cli._apply_relocalise(base(), parse(["--relocalise", "--relocalise-keypoint-levels", "0"]))
    assert said is not None and "relocalise_keypoint_levels" in said
    with pytest.raises(SystemExit):
        parse(["--relocalise", "--relocalise-search", "orb"])
    with pytest.raises(SystemExit):
        parse(["--loop-closure", "--loop-closure-candidates", "orb"])


def print_figures():
    for yaw, back in FAR_TABLE:
        A = view_pose(yaw)
        B = moved_back(A, back)
        row = f"yaw {yaw:3g}  {back} m back  centre depth {centre_depth(A):.2f} -> {centre_depth(B):.2f} ({centre_depth(B) / centre_depth(A):.2f})"
        for L in (1, 3, 5):
            n, inl, T, want = reference_pose(A, B, L)
            off = "-" if T is None else f"{1e3 * np.linalg.norm(T[:3, 3] - want[:3, 3]):.1f} mm"
            row += f"   {L} levels: {n} / {inl}, {off}"
        print(row)
    for y0 in (0.0, 50.0, 120.0):
        n, inl, _, _ = reference_pose(view_pose(y0), moved_back(view_pose(y0), 1.2), 3)
        print(f"yaw {y0:g}, 1.2 m back, 3 levels: {n} matches / {inl} inliers")
    for turn in (90.0, 180.0):
        for back in (0.0, 1.2):
            n, inl, _, _ = reference_pose(view_pose(0.0), moved_back(view_pose(turn), back), 3)
            print(f"wrong: the wall {turn:g} degrees on, {back} m back, 3 levels: {n} matches / {inl} inliers")
    for pair in FAR_PAIRS:
        score, rel, (n1, i1, _, _), (n3, i3, T3, want) = far_pair_figures(pair)
        print(f"far turn {pair}: score {score:.4f} depth_rel {rel:.4f}  1 level {n1} / {i1}  3 levels {n3} / {i3}  pose off "
              f"{1e3 * np.linalg.norm(T3[:3, 3] - want[:3, 3]):.1f} mm {angle_deg(pg.inverse(want) @ T3):.2f} deg")


if __name__ == "__main__":
    print_figures()
