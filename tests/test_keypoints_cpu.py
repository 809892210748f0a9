"""tests/keypoint_reference.py, the definition of the keypoint registration, on hand-made cases; and, on the CPU, what it is for: a
revisit in the textured box room that lies beyond the correction gate of the yaw guess and registers from the keypoint pose.

THE TEXTURED ROOM: synth.box_room_texture_color (cell 0.2 m, amplitude 0.12) with CAM and CENTRE of tests/test_loop_closure_gpu.py.

Measured with the definition at the defaults (`python -m tests.test_keypoints_cpu` prints it), from the view at CENTRE, yaw 0:
    pair                                   keypoints   matches   inliers   error of the RANSAC pose
    54 mm / 3 deg apart                    151 / 149      72        72      1.9 mm, 0.04 deg
    0.3 m / 10 deg apart                   151 / 152      42        34     10.5 mm, 0.20 deg
    0.5 m / 12 deg apart, 8 deg roll       151 / 154      36        23     12.5 mm, 0.24 deg
    the wall 90 deg to the right           151 /  98      13         1     -
    the opposite wall                      151 / 161      18         1     -
and over six more starting yaws: right pairs 18 - 81 inliers, wrong pairs at most 1.  min_inliers stays 8.

THE WIDE TURN (shared with tests/test_keypoints_gpu.py and tests/test_loop_closure_keypoints_gpu.py): the turn of
tests/test_place_cpu.py in the textured room, its revisit frames 36 .. 41 moved to WIDE_OFFSET = (0.3, -0.05, 0) m, 6 degrees of
yaw and 3 degrees of roll - 304 mm.  (The issue's 0.4 m / 6 degrees / 5 degrees of roll scores 0.88 and 0.85 on the thumbnails of
this texture, below loop_closure_min_score; this offset was chosen on the CPU as the widest of those tried at which both wide
pairs stay appearance candidates.)  With the definitions, S = 4, tw = 40:
    pair      score    shift   depth_rel   matches   inliers   keypoint pose off by   yaw guess off by
    (0, 12)   0.9406    +4      0.0546        57        53      6.8 mm, 0.11 deg       0.0 mm, 1.31 deg     (frame 35: not moved)
    (1, 13)   0.9233    -4      0.0457        59        49      2.9 mm, 0.03 deg     304.1 mm, 6.10 deg
    (2, 14)   0.9104    -4      0.0695        49        40      6.4 mm, 0.24 deg     304.1 mm, 6.10 deg
    every other pair: score <= 0.8672
From the keypoint pose tests/rgbd_align_reference.refine lands 0.89 and 0.52 mm from the truth on the wide pairs and every gate of
register_pair passes; from the yaw guess it lands in the same place and is refused: correction 0.304 m / 6.1 degrees."""
import numpy as np
import pytest

from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import pose_graph as pg
from rtg_slam_amd import synth
from rtg_slam_amd.rgbd_align import se3_exp
from tests import keypoint_reference as ref
from tests.test_loop_closure_gpu import CAM, CENTRE, loop_args
from tests.test_place_cpu import FRAMES, KEYFRAMES, REVISIT_FROM, NumpyRefiner, angle_deg

F32 = np.float32
K_CAM = np.array([[CAM.fx, 0, CAM.cx], [0, CAM.fy, CAM.cy], [0, 0, 1.0]])
WIDE_OFFSET, WIDE_YAW_DEG, WIDE_ROLL_DEG = (0.3, -0.05, 0.0), 6.0, 3.0
WIDE_PAIRS = ((1, 13), (2, 14))                                   # keyframe pairs of the wide turn beyond the yaw guess's gate


def image_of(g8):
    """A colour image whose 8-bit grey value is exactly g8."""
    g = g8.astype(F32) / F32(255)
    c = np.stack([g, g, g])
    assert np.array_equal(ref.grey8(c), g8)
    return c


def dots(H, W, at, dark=40, bright=200):
    g = np.full((H, W), dark, np.uint8)
    for x, y in at:
        g[y, x] = bright
    return g


def keypoints_of(g8, depth=None, **kw):
    depth = np.ones(g8.shape, F32) if depth is None else depth
    s = ref.detect(image_of(g8), depth, **kw)[2]
    return [tuple(int(v) for v in r[:3]) for r in s if r[2] > 0]


def view_pose(yaw_deg, offset=(0.0, 0.0, 0.0), roll_deg=0.0):
    T = se3_exp([0.0, np.deg2rad(yaw_deg), 0.0, 0.0, 0.0, 0.0]) @ se3_exp([0.0, 0.0, np.deg2rad(roll_deg), 0.0, 0.0, 0.0])
    T[:3, 3] = np.asarray(CENTRE) + np.asarray(offset)
    return T


_cache = {}


def textured_view(T):
    """(depth [H, W, 1], colour [3, H, W]) CPU tensors of the textured room seen from c2w T; rendered once per pose."""
    import torch
    key = ("view", np.asarray(T).tobytes())
    if key not in _cache:
        p = torch.from_numpy(np.asarray(T))
        d = synth.box_room_depth(CAM, p)
        _cache[key] = (d, synth.box_room_texture_color(CAM, p, d))
    return _cache[key]


def features_of(T):
    """The definition's features of the textured view at T, with "xyz"; computed once per pose."""
    key = ("feat", np.asarray(T).tobytes())
    if key not in _cache:
        d, c = textured_view(T)
        z = d.numpy().reshape(CAM.H, CAM.W)
        f = ref.detect_and_describe(c.numpy(), z)
        f["xyz"] = ref.backproject(f["x"], f["y"], z, K_CAM)
        _cache[key] = f
    return _cache[key]


def reference_pose(Ta, Tb, min_inliers=8):
    """-> (matches, inliers, T or None, the true T_a^-1 T_b) by the definition alone."""
    fa, fb = features_of(Ta), features_of(Tb)
    m = ref.filter_matches(ref.match(fb["desc"], fa["desc"]), ref.match(fa["desc"], fb["desc"]))
    want = pg.inverse(Ta) @ Tb
    fit = ref.ransac_rigid(fa["xyz"][[j for _, j, _ in m]], fb["xyz"][[i for i, _, _ in m]]) if len(m) >= 3 else None
    if fit is None:
        return len(m), 0, None, want
    return len(m), int(fit[1].sum()), fit[0], want


def wide_turn_poses():
    out = []
    for k in range(FRAMES):
        late = k >= REVISIT_FROM
        T = view_pose(10.0 * k + (WIDE_YAW_DEG if late else 0.0), WIDE_OFFSET if late else (0.0, 0.0, 0.0), WIDE_ROLL_DEG if late else 0.0)
        out.append(T)
    return out


def wide_turn_frames():
    """[(depth, colour, true c2w)] of the 42 frames of the wide turn as CPU tensors, rendered once."""
    if "turn" not in _cache:
        _cache["turn"] = [textured_view(T) + (T,) for T in wide_turn_poses()]
    return _cache["turn"]


# ---- 1. detection on hand-made images ----

def test_a_bright_square_yields_exactly_its_four_corners():
    g = np.full((80, 96), 40, np.uint8)
    g[28:52, 36:60] = 200                                         # corners (36, 28), (59, 28), (36, 51), (59, 51)
    # the few pixels at a corner tie at 160; the raster-order rule keeps the first of each run: edges and interior score 0
    assert keypoints_of(g) == [(36, 28, 160), (57, 28, 160), (36, 49, 160), (59, 49, 160)]
    s = ref.fast_score(g)
    assert s[28, 40:56].max() == 0 and s[31:49, 36].max() == 0 and s[31:49, 39:57].max() == 0     # an edge, an edge, the interior


def test_a_constant_image_and_an_image_without_depth_yield_nothing():
    assert keypoints_of(np.full((48, 64), 90, np.uint8)) == []
    g = dots(48, 64, [(20, 20), (40, 25)])
    assert keypoints_of(g) == [(20, 20, 160), (40, 25, 160)]
    assert keypoints_of(g, np.zeros((48, 64), F32)) == []
    z = np.ones((48, 64), F32)
    z[20, 20], z[25, 40] = np.nan, -1.0
    assert keypoints_of(g, z) == []
    z[20, 20], z[25, 40] = np.inf, 0.5
    assert keypoints_of(g, z) == [(40, 25, 160)]


def test_the_margin_keeps_16_and_drops_15():
    assert keypoints_of(dots(80, 96, [(16, 30)])) == [(16, 30, 160)]
    assert keypoints_of(dots(80, 96, [(15, 30)])) == []
    assert keypoints_of(dots(80, 96, [(79, 63)])) == [(79, 63, 160)]            # W - 17, H - 17: the last pixel inside
    assert keypoints_of(dots(80, 96, [(80, 40)])) == [] and keypoints_of(dots(80, 96, [(40, 64)])) == []
    assert keypoints_of(dots(80, 96, [(40, 15)])) == []


def test_the_threshold_is_exclusive():
    g = dots(48, 64, [(20, 20)], dark=40, bright=60)              # score 20
    assert keypoints_of(g) == [] and keypoints_of(g, threshold=19) == [(20, 20, 20)]


def test_ties_two_equal_maxima_in_one_cell_and_equal_neighbours():
    # one cell (16 .. 31 both ways), two dots of the same score: the lower row-major index wins
    assert keypoints_of(dots(64, 64, [(26, 22), (20, 20)])) == [(20, 20, 160)]
    assert keypoints_of(dots(64, 64, [(20, 22), (26, 20)])) == [(26, 20, 160)]
    # equal scores on neighbouring pixels: the one earlier in raster order survives, the later one does not
    for pair, kept in ((((20, 20), (21, 20)), (20, 20)), (((20, 20), (20, 21)), (20, 20)), (((21, 20), (20, 21)), (21, 20)),
                       (((20, 20), (21, 21)), (20, 20))):
        g = dots(64, 64, pair)
        s = ref.eligible_score(g, np.ones((64, 64), F32), 20)
        assert s[pair[0][1], pair[0][0]] == s[pair[1][1], pair[1][0]] > 0
        assert keypoints_of(g) == [kept + (int(s[kept[1], kept[0]]),)]
    # a pair that straddles two cells: the suppression looks across the cell's edge
    assert keypoints_of(dots(64, 64, [(31, 20), (32, 20)])) == [(31, 20, 160)]


def test_partial_cells():
    H, W = 83, 101
    g = dots(H, W, [(84, 60), (20, 20)])
    s = ref.detect(image_of(g), np.ones((H, W), F32))[2]
    assert s.shape == (7 * 6, 4)                                  # ceil(101 / 16) x ceil(83 / 16)
    assert [tuple(r) for r in s if r[2] > 0] == [(20, 20, 160, -1), (84, 60, 160, -1)]
    assert (s[6::7, 2] == 0).all() and (s[35:, 2] == 0).all()      # at 16 the partial cells lie inside the margin: always empty
    s = ref.detect(image_of(g), np.ones((H, W), F32), cell=28)[2]   # cells of 28: the last column is 84 .. 100, the last row 56 .. 82
    assert s.shape == (4 * 3, 4) and tuple(s[2 * 4 + 3]) == (84, 60, 160, -1) and tuple(s[0]) == (20, 20, 160, -1)


# ---- 2. orientation and descriptor ----

def test_the_orientation_needs_int64():
    g = np.zeros((64, 64), np.uint8)
    g[:, 33:] = 255                                               # bright to the right of the keypoint at (32, 32)
    g[40:, :] = 255                                               # and below
    m10, m01 = ref.moments(g, 32, 32)
    dirs = ref.direction_table()
    v = dirs[:, 0].astype(np.int64) * m10 + dirs[:, 1].astype(np.int64) * m01
    assert np.abs(v).max() > 2 ** 31 and m10 > 0 and m01 > 0
    k = ref.orientation_bin(m10, m01)
    assert k == int(np.rint(np.arctan2(m01, m10) / (2 * np.pi / 32))) % 32
    wrapped = v.astype(np.int32)                                  # what 32-bit sums of products would hold
    assert int(np.argmax(wrapped)) != k
    assert ref.orientation_bin(0, 0) == 0 and ref.orientation_bin(5, 0) == 0 and ref.orientation_bin(0, 5) == 8
    assert ref.orientation_bin(16069, 3196) == 1                  # (C_1, S_1): ties between bins go to the lower one below
    assert ref.orientation_bin(1, 1) == 4 and ref.orientation_bin(-3, 0) == 16 and ref.orientation_bin(0, -2) == 24


def test_the_tables_are_the_packages_and_stay_within_13():
    from rtg_slam_amd import keypoints as kp
    t = ref.rotated_patterns()
    assert np.array_equal(t, kp.rotated_patterns()) and np.array_equal(ref.direction_table(), kp.direction_table())
    assert t.shape == (32, 256, 4) and t.dtype == np.int8
    tt = t.astype(np.int64)
    assert (tt[0, :, 0] ** 2 + tt[0, :, 1] ** 2 <= 169).all() and (tt[0, :, 2] ** 2 + tt[0, :, 3] ** 2 <= 169).all()
    assert np.abs(tt).max() <= 13                                 # turned and rounded: within +-13, so every read within the margin
    assert np.array_equal(t[0], np.asarray(ref.PATTERN, dtype=np.int8))
    assert np.array_equal(t[8, :, 0], -t[0, :, 1]) and np.array_equal(t[8, :, 1], t[0, :, 0])       # a quarter turn, exactly
    assert len(set(ref.PATTERN)) == 256
    assert ref.mix32(0) == kp.mix32(0) and [ref.mix32(i) for i in range(1, 50)] == [kp.mix32(i) for i in range(1, 50)]


def test_an_image_and_its_rot90():
    rng = np.random.default_rng(5)
    g = np.kron(rng.integers(30, 226, size=(12, 12)).astype(np.uint8), np.ones((10, 10), np.uint8))      # 120 x 120, blocks of 10
    z = np.ones((120, 120), F32)
    f0 = ref.detect_and_describe(image_of(g), z)
    f1 = ref.detect_and_describe(image_of(np.rot90(g).copy()), z)
    # np.rot90 turns counter-clockwise: the pixel (x, y) goes to (y, W - 1 - x)
    at = {(int(y), int(119 - x)): k for k, (x, y) in enumerate(zip(f0["x"], f0["y"]))}
    both = [(at[(int(x), int(y))], k) for k, (x, y) in enumerate(zip(f1["x"], f1["y"])) if (int(x), int(y)) in at]
    assert len(both) >= 5, (len(f0["x"]), len(f1["x"]), len(both))   # the tie rules and the cells are not turned: some differ
    for k0, k1 in both:
        assert (int(f0["bin"][k0]) - int(f1["bin"][k1])) % 32 == 8
        assert np.array_equal(f0["desc"][k0], f1["desc"][k1]) and f0["score"][k0] == f1["score"][k1]
    flat = ref.detect_and_describe(image_of(g), z, oriented=False)
    assert (flat["bin"] == 0).all() and np.array_equal(flat["x"], f0["x"]) and not np.array_equal(flat["desc"], f0["desc"])


# ---- 3. match and filter ----

def random_desc(n, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)


def brute_match(q, r):
    out = []
    for a in q:
        d = [sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b)) for b in r]
        if not d:
            out.append((-1, 257, 257))
            continue
        j = min(range(len(d)), key=lambda i: (d[i], i))
        out.append((j, d[j], min([x for i, x in enumerate(d) if i != j], default=257)))
    return np.asarray(out, dtype=np.int32).reshape(-1, 3)


@pytest.mark.parametrize("nq,nr", [(1, 1), (5, 0), (130, 65)])
def test_match_sizes(nq, nr):
    q, r = random_desc(nq, 1), random_desc(nr, 2)
    if nr:
        r[::7] = q[:len(r[::7])]                                  # some exact hits
    got = ref.match(q, r)
    assert got.dtype == np.int32 and np.array_equal(got, brute_match(q, r))
    if nr == 0:
        assert (got == (-1, 257, 257)).all()
    if nr == 1:
        assert got[0, 0] == 0 and got[0, 2] == 257


def test_match_ties_and_the_last_bit():
    q = random_desc(3, 3)
    same = np.repeat(q[:1], 6, axis=0)
    assert np.array_equal(ref.match(q[:1], same), [[0, 0, 0]])     # all identical: index 0, second = best
    a = np.zeros((1, 8), np.uint32)
    b = a.copy()
    b[0, 7] = np.uint32(1) << np.uint32(31)                        # differs only in bit 255
    assert ref.hamming(a, b)[0, 0] == 1
    assert np.array_equal(ref.match(a, np.concatenate([b, a, b])), [[1, 0, 1]])
    assert np.array_equal(ref.match(a, np.concatenate([b, b])), [[0, 1, 1]])


def test_filter_mutual_hamming_and_ratio():
    m_ba = np.array([[0, 10, 40], [1, 10, 12], [2, 70, 200], [0, 5, 100], [-1, 257, 257]], np.int32)   # b's five against a's three
    m_ab = np.array([[3, 5, 9], [1, 10, 50], [2, 70, 90]], np.int32)
    # 0: a's 0 prefers b's 3; 1: 10 > 0.8 x 12; 2: 70 > 64; 3: mutual, 5 <= 80; 4: nothing
    assert ref.filter_matches(m_ba, m_ab) == [(3, 0, 5)]
    assert ref.filter_matches(m_ba, m_ab, max_hamming=70, ratio=0.9) == [(1, 1, 10), (2, 2, 70), (3, 0, 5)]
    from rtg_slam_amd import keypoints as kp
    assert kp.filter_matches(m_ba, m_ab, 70, 0.9) == ref.filter_matches(m_ba, m_ab, 70, 0.9)


# ---- 4. the rigid pose ----

def test_ransac_recovers_the_pose_under_gross_outliers_and_repeats():
    from rtg_slam_amd import keypoints as kp
    rng = np.random.default_rng(7)
    T = se3_exp([0.1, -0.3, 0.05, 0.4, -0.2, 0.3])
    pb = rng.uniform(-2, 2, size=(50, 3)) + (0, 0, 3)
    pa = pb @ T[:3, :3].T + T[:3, 3]
    bad = rng.permutation(50)[:20]                                 # 40 % gross outliers
    pa[bad] += rng.uniform(0.5, 2.0, size=(20, 3)) * rng.choice([-1, 1], size=(20, 3))
    got, mask, rms = ref.ransac_rigid(pa, pb)
    assert np.abs(got - T).max() < 1e-9 and mask.sum() == 30 and not mask[bad].any() and rms < 1e-9
    again = ref.ransac_rigid(pa, pb)
    assert np.array_equal(again[0], got) and np.array_equal(again[1], mask) and again[2] == rms
    mine = kp.ransac_rigid(pa, pb)                                 # the package's copy is the same function
    assert np.array_equal(mine[0], got) and np.array_equal(mine[1], mask) and mine[2] == rms


def test_ransac_refuses_two_matches_and_collinear_points():
    p = np.array([[0, 0, 1.0], [1, 0, 1], [0, 1, 2]])
    assert ref.ransac_rigid(p[:2], p[:2]) is None
    assert ref.ransac_rigid(p, p) is not None
    line = np.outer(np.linspace(0, 3, 12), [1.0, 0.5, 0.2]) + (0, 0, 2)
    assert ref.ransac_rigid(line, line) is None
    near = line.copy()
    near[:, 1] += 1e-3 * np.sin(np.arange(12))                     # 1 mm off a 3.4 m line: below the rule's 5.74 degrees
    assert ref.ransac_rigid(near, near) is None


# ---- 5. the textured room ----

RIGHT = {"54 mm / 3 deg": (3.0, (0.04, -0.02, 0.03), 0.0), "0.3 m / 10 deg": (10.0, (0.2, -0.1, 0.2), 0.0),
         "0.5 m / 12 deg, 8 deg roll": (12.0, (0.35, -0.1, 0.34), 8.0)}
WRONG = {"the wall to the right": 90.0, "the opposite wall": 180.0}


@pytest.mark.parametrize("name", sorted(RIGHT))
def test_right_pairs_have_their_inliers_and_a_pose_inside_the_gate(name):
    yaw, off, roll = RIGHT[name]
    cfg = lc.LoopCloser(loop_args())
    n, inl, T, want = reference_pose(view_pose(0.0), view_pose(yaw, off, roll))
    err, ang = float(np.linalg.norm(T[:3, 3] - want[:3, 3])), angle_deg(pg.inverse(want) @ T)
    print(f"{name}: {n} matches, {inl} inliers, {1e3 * err:.1f} mm / {ang:.2f} degrees from the truth")
    assert inl >= cfg.keypoints.cfg.min_inliers == 8
    assert err <= cfg.cfg.max_correction_trans and ang <= cfg.cfg.max_correction_rot_deg


@pytest.mark.parametrize("name", sorted(WRONG))
def test_wrong_pairs_end_below_min_inliers(name):
    n, inl, _, _ = reference_pose(view_pose(0.0), view_pose(WRONG[name]))
    print(f"{name}: {n} matches, {inl} inliers")
    assert n >= 3 and inl < 8


def wide_pyramids(k):
    import torch
    from oracle import icp_oracle as io
    from tests import rgbd_align_reference as rar
    key = ("pyr", k)
    if key not in _cache:
        d, c, _ = wide_turn_frames()[KEYFRAMES[k]]
        vp = io.vertex_pyramid(d, torch.tensor(K_CAM, dtype=torch.float32), 3)
        _cache[key] = {"vertex": [x.numpy() for x in vp], "normal": [x.numpy() for x in io.normal_pyramid(vp)],
                       "intensity": rar.intensity_pyramid(c.numpy(), 3)}
    return _cache[key]


def wide_pair_figures(pair):
    """The thumbnails' verdict, the yaw guess and the keypoint pose of a keyframe pair of the wide turn, by the definitions."""
    from tests import place_reference as pref
    a, b = pair
    fr = wide_turn_frames()
    A, B = (pref.describe(fr[KEYFRAMES[k]][1].numpy(), fr[KEYFRAMES[k]][0].numpy(), 40) for k in (a, b))
    sc, sh, rel = pref.pair_scores(A[0][None], A[1][None], A[2][None], B[0][None], B[1][None], B[2][None], 4)
    n, inl, T, want = reference_pose(fr[KEYFRAMES[a]][2], fr[KEYFRAMES[b]][2])
    return float(sc[0]), int(sh[0]), float(rel[0]), pref.appearance_init(int(sh[0]), CAM.fx, CAM.W, 40), n, inl, T, want


@pytest.mark.parametrize("pair", WIDE_PAIRS)
def test_the_wide_revisit_registers_from_the_keypoint_pose_and_not_from_the_yaw_guess(pair):
    cfg = lc.LoopCloser(loop_args()).cfg
    score, shift, rel, yaw, n, inl, T, want = wide_pair_figures(pair)
    assert score >= 0.9 and rel <= 0.1 and inl >= 8                # an appearance candidate at the defaults, with its witnesses
    Kf = K_CAM.astype(F32)
    for name, init in (("keypoints", T), ("yaw", yaw)):
        r = lc.register_pair(NumpyRefiner(), wide_pyramids(pair[1]), wide_pyramids(pair[0]), init, Kf, [0.25, 0.5, 1.0], cfg)
        err = float(np.linalg.norm(r["Z"][:3, 3] - want[:3, 3]))
        print(f"{pair} from {name}: score {score:.4f}, shift {shift:+d}, depth_rel {rel:.4f}, {n} matches, {inl} inliers; guess off by "
              f"{1e3 * np.linalg.norm(init[:3, 3] - want[:3, 3]):.1f} mm / {angle_deg(pg.inverse(want) @ init):.2f} degrees -> "
              f"{r['reason']}, {1e3 * err:.2f} mm from the truth, inlier ratio {r['inlier_ratio']:.3f}")
        if name == "keypoints":
            assert r["accepted"], r["reason"]
            assert err < 5e-3
        else:
            assert not r["accepted"] and r["reason"].startswith("correction "), r["reason"]


# ---- 6. the keys ----

def test_the_new_keys_default_to_yaw_and_are_validated():
    closer = lc.LoopCloser(loop_args())
    assert closer.keypoints.init == "yaw"
    assert vars(closer.keypoints.cfg) == dict(threshold=20, cell=16, oriented=True, max_hamming=64, ratio=0.8, ransac_iters=512,
                                              inlier_dist=0.05, min_inliers=8)
    assert not any(k.startswith("keypoint") or k == "init" for k in list(vars(closer.cfg)) + list(vars(closer.place)))
    assert not hasattr(loop_args(), "loop_closure_appearance_init")
    ok = dict(loop_closure_candidates="appearance", loop_closure_appearance_init="keypoints")
    lc.LoopCloser(loop_args(**ok))
    lc.LoopCloser(loop_args(loop_closure_candidates="both", loop_closure_appearance_init="keypoints_strict"))
    lc.LoopCloser(loop_args(loop_closure_candidates="pose", loop_closure_appearance_init="yaw"))
    for over in (dict(loop_closure_appearance_init="keypoints"), dict(loop_closure_candidates="pose", loop_closure_appearance_init="keypoints_strict"),
                 dict(ok, loop_closure_appearance_init="orb"), dict(ok, loop_closure_keypoint_threshold=-1),
                 dict(ok, loop_closure_keypoint_threshold=256), dict(ok, loop_closure_keypoint_cell=7), dict(ok, loop_closure_keypoint_cell=33),
                 dict(ok, loop_closure_keypoint_max_hamming=257), dict(ok, loop_closure_keypoint_ratio=0.0),
                 dict(ok, loop_closure_keypoint_ratio=1.5), dict(ok, loop_closure_keypoint_ransac_iters=0),
                 dict(ok, loop_closure_keypoint_inlier_dist=0.0), dict(ok, loop_closure_keypoint_min_inliers=2),
                 dict(loop_closure_keypoint_cell=7)):
        with pytest.raises(ValueError):
            lc.LoopCloser(loop_args(**over))


def test_the_cli_flags_set_the_keys_only_when_given():
    from types import SimpleNamespace
    from rtg_slam_amd import __main__ as cli
    parse = lambda argv: cli.build_parser().parse_args(["slam", "--config", "x.yaml"] + argv)
    args = SimpleNamespace()
    assert cli._apply_loop_closure(args, parse(["--loop-closure", "--loop-closure-candidates", "appearance", "--loop-closure-appearance-init",
                                                "keypoints", "--loop-closure-keypoint-oriented", "false", "--loop-closure-keypoint-cell", "24",
                                                "--loop-closure-keypoint-min-inliers", "12", "--loop-closure-keypoint-ratio", "0.7"])) is None
    assert vars(args) == dict(loop_closure=True, loop_closure_candidates="appearance", loop_closure_appearance_init="keypoints",
                              loop_closure_keypoint_oriented=False, loop_closure_keypoint_cell=24, loop_closure_keypoint_min_inliers=12,
                              loop_closure_keypoint_ratio=0.7)
    closer = lc.LoopCloser(args)
    assert closer.keypoints.init == "keypoints" and closer.keypoints.cfg.oriented is False and closer.keypoints.cfg.cell == 24
    for name in lc.DEFAULTS:                                      # every key has its flag
        if name.startswith("loop_closure_keypoint_") or name == "loop_closure_appearance_init":
            assert any("loop_closure_" + flag == name for flag, *_ in cli.LOOP_CLOSURE_FLAGS), name
    said = cli._apply_loop_closure(SimpleNamespace(), parse(["--loop-closure", "--loop-closure-appearance-init", "keypoints"]))
    assert said is not None and "appearance or both" in said
    said = cli._apply_loop_closure(SimpleNamespace(), parse(["--loop-closure-appearance-init", "keypoints"]))
    assert said is not None and "needs --loop-closure" in said
    said = cli._apply_loop_closure(SimpleNamespace(), parse(["--loop-closure", "--loop-closure-keypoint-cell", "4"]))
    assert said is not None and "loop_closure_keypoint_cell" in said
    with pytest.raises(SystemExit):
        parse(["--loop-closure", "--loop-closure-appearance-init", "orb"])


def test_the_textured_room_is_the_smooth_room_plus_a_bounded_offset():
    import torch
    T = torch.from_numpy(view_pose(20.0))
    d = synth.box_room_depth(CAM, T)
    smooth, tex = synth.box_room_color(CAM, T, d), synth.box_room_texture_color(CAM, T, d)
    assert tex.shape == smooth.shape and tex.dtype == torch.float32 and float(tex.min()) >= 0 and float(tex.max()) <= 1
    off = (tex - smooth)
    assert float(off.abs().max()) <= 0.12 + 1e-6 and float(off.abs().max()) > 0.08
    inside = (smooth > 0.13) & (smooth < 0.87)                    # where nothing was clamped the three channels got one offset
    same = ((off[0] - off[1]).abs() < 1e-6) & ((off[0] - off[2]).abs() < 1e-6)
    assert bool(same[inside.all(dim=0)].all())
    assert torch.equal(synth.box_room_texture_color(CAM, T, d, amplitude=0.0), smooth)
    assert len(torch.unique(torch.round(off[0][inside.all(dim=0)] * 1e4))) > 20       # many cells, each its own level


def print_figures():
    for y0 in (0, 20, 50, 90, 140, 200, 290):
        for name, (yaw, off, roll) in RIGHT.items():
            n, inl, T, want = reference_pose(view_pose(y0), view_pose(y0 + yaw, off, roll))
            print(f"yaw {y0:3d} {name:28s} {n:3d} matches {inl:3d} inliers  {1e3 * np.linalg.norm(T[:3, 3] - want[:3, 3]):5.1f} mm "
                  f"{angle_deg(pg.inverse(want) @ T):.2f} deg")
        for name, yaw in WRONG.items():
            n, inl, _, _ = reference_pose(view_pose(y0), view_pose(y0 + yaw))
            print(f"yaw {y0:3d} {name:28s} {n:3d} matches {inl:3d} inliers")
    for pair in ((0, 12),) + WIDE_PAIRS:
        score, shift, rel, yaw, n, inl, T, want = wide_pair_figures(pair)
        print(pair, f"score {score:.4f} shift {shift:+d} depth_rel {rel:.4f} matches {n} inliers {inl} keypoint pose off "
              f"{1e3 * np.linalg.norm(T[:3, 3] - want[:3, 3]):.1f} mm {angle_deg(pg.inverse(want) @ T):.2f} deg; yaw guess off "
              f"{1e3 * np.linalg.norm(yaw[:3, 3] - want[:3, 3]):.1f} mm {angle_deg(pg.inverse(want) @ yaw):.2f} deg")


if __name__ == "__main__":
    print_figures()
