"""csrc/keypoints.hip against tests/keypoint_reference.py: rtgs_keypoint_detect, rtgs_keypoint_describe and rtgs_keypoint_match are
integer arithmetic after the grey value, so every comparison here is np.array_equal / torch.equal."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import keypoints as kp
from tests import keypoint_reference as ref
from tests.test_keypoints_cpu import (K_CAM, WIDE_PAIRS, brute_match, dots, features_of, image_of, random_desc, textured_view, view_pose,
                                      wide_turn_frames)
from tests.test_loop_closure_gpu import CAM, DEV
from tests.test_place_cpu import KEYFRAMES

pytestmark = pytest.mark.gpu
F32 = np.float32
K_SMALL = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]])


def blocks_image(H, W, seed, block=7):
    """Colour blocks with a little per-pixel noise (so that the float32 grey chain and its rounding matter) and a depth with
    holes, NaN and inf in it."""
    rng = np.random.default_rng(seed)
    by, bx = -(-H // block), -(-W // block)
    c = np.kron(rng.random((3, by, bx)), np.ones((block, block)))[:, :H, :W] * 0.9 + rng.random((3, H, W)) * 0.1
    z = 1.0 + rng.random((H, W))
    bad = rng.random((H, W))
    z[bad < 0.05] = 0.0
    z[(bad >= 0.05) & (bad < 0.07)] = np.nan
    z[(bad >= 0.07) & (bad < 0.09)] = np.inf
    z[(bad >= 0.09) & (bad < 0.11)] = -1.0
    return c.astype(F32), z.astype(F32)


def device_features(color, depth, K=K_SMALL, **over):
    f = kp.detect_and_describe(torch.from_numpy(np.ascontiguousarray(color)).to(DEV), torch.from_numpy(np.ascontiguousarray(depth)).to(DEV)[None],
                               K, kp.config(**over), keep_planes=True)
    torch.cuda.synchronize()
    return f


def words(t):
    """int32 device words -> the uint32 numpy array of the definition."""
    return t.cpu().numpy().view(np.uint32)


def assert_equal_features(f, want, depth, K):
    assert np.array_equal(f["g8"].cpu().numpy(), want["g8"])
    assert np.array_equal(f["box5"].cpu().numpy(), want["box5"])
    assert np.array_equal(f["slots"].cpu().numpy(), want["slots"])
    assert np.array_equal(words(f["slot_desc"]), want["slot_desc"])
    for k in ("x", "y", "score", "bin"):
        assert f[k].dtype == np.int32 and np.array_equal(f[k], want[k]), k
    assert np.array_equal(words(f["desc"]).reshape(-1, 8), want["desc"].reshape(-1, 8))
    xyz = ref.backproject(want["x"], want["y"], np.asarray(depth).reshape(want["g8"].shape), K)
    assert f["xyz"].dtype == np.float64 and np.array_equal(f["xyz"], xyz)


@pytest.mark.parametrize("H,W,over", [(48, 64, {}), (48, 64, dict(cell=8)), (83, 101, {}), (83, 101, dict(cell=28, threshold=10)), (83, 101, dict(cell=8)),
                                      (48, 64, dict(cell=32, oriented=False))])
def test_detect_and_describe_match_the_definition(H, W, over):
    color, depth = blocks_image(H, W, H + W)
    f = device_features(color, depth, **over)
    cfg = kp.config(**over)
    want = ref.detect_and_describe(color, depth, cfg.threshold, cfg.cell, cfg.oriented)
    print(f"{W} x {H} {over}: {len(want['x'])} keypoints in {want['slots'].shape[0]} slots, bins {sorted(set(want['bin'].tolist()))[:6]} ..")
    assert len(want["x"]) >= 2                                    # 64 x 48 at cell 16: the margin leaves two cells
    assert_equal_features(f, want, depth, K_SMALL)
    if not cfg.oriented:
        assert (f["bin"] == 0).all()


def test_a_textured_view_matches_the_definition():
    T = view_pose(20.0)
    d, c = textured_view(T)
    f = kp.detect_and_describe(c.to(DEV), d.to(DEV).reshape(1, CAM.H, CAM.W), K_CAM, keep_planes=True)
    want = features_of(T)
    print(f"320 x 240: {len(want['x'])} keypoints, scores {want['score'].min()} .. {want['score'].max()}, {len(set(want['bin'].tolist()))} bins")
    assert len(want["x"]) > 100
    assert_equal_features(f, want, d.numpy(), K_CAM)
    assert np.array_equal(f["xyz"], want["xyz"])


def test_hand_made_cases_on_the_device():
    for g in (dots(64, 64, [(26, 22), (20, 20)]), dots(64, 64, [(20, 22), (26, 20)]), dots(64, 64, [(21, 20), (20, 21)]),
              dots(64, 64, [(31, 20), (32, 20)]), dots(80, 96, [(16, 30), (15, 50), (79, 63), (80, 40)])):
        z = np.ones(g.shape, F32)
        want = ref.detect_and_describe(image_of(g), z)
        assert_equal_features(device_features(image_of(g), z), want, z, K_SMALL)
    sq = np.full((80, 96), 40, np.uint8)
    sq[28:52, 36:60] = 200
    f = device_features(image_of(sq), np.ones(sq.shape, F32))
    assert list(zip(f["x"].tolist(), f["y"].tolist(), f["score"].tolist())) == [(36, 28, 160), (57, 28, 160), (36, 49, 160), (59, 49, 160)]


def test_the_empty_cases():
    flat = np.full((3, 48, 64), 0.4, F32)
    f = device_features(flat, np.ones((48, 64), F32))
    assert f["x"].shape == (0,) and tuple(f["desc"].shape) == (0, 8) and f["xyz"].shape == (0, 3)
    assert np.array_equal(f["slots"].cpu().numpy(), np.tile(np.array([0, 0, 0, -1], np.int32), (12, 1))) and not f["slot_desc"].any()
    g = dots(48, 64, [(20, 20), (40, 25)])
    assert len(device_features(image_of(g), np.ones((48, 64), F32))["x"]) == 2
    f0 = device_features(image_of(g), np.zeros((48, 64), F32))
    assert len(f0["x"]) == 0 and np.array_equal(f0["g8"].cpu().numpy(), g)
    nan = image_of(g)
    nan[:, 5, 5] = np.nan                                         # a NaN colour is grey 0
    assert device_features(nan, np.ones((48, 64), F32))["g8"][5, 5].item() == 0
    # matching against nothing, and nothing against something: one launch each, no keypoint needed
    some = {"desc": torch.from_numpy(random_desc(5, 1).view(np.int32)).to(DEV)}
    a, b = kp.match_pairs({"e": f0, "s": some}, [("s", "e"), ("e", "s")])
    assert np.array_equal(a, np.tile(np.array([-1, 257, 257], np.int32), (5, 1))) and b.shape == (0, 3)
    assert kp.match_pairs({"e": f0}, [("e", "e")])[0].shape == (0, 3) and kp.match_pairs({}, []) == []
    r = kp.relative_pose(f0, f0)
    assert r["T"] is None and r["reason"] == "0 inliers of 0 matches, below 8" and r["matches"] == 0 and r["keypoints_a"] == 0


def test_the_orientation_is_int64_on_the_device():
    """The definition's case whose products pass 2^31, through rtgs_keypoint_describe with a hand-made slot."""
    from rtg_slam_amd import _lib
    g = np.zeros((64, 64), np.uint8)
    g[:, 33:] = 255
    g[40:, :] = 255
    box = ref.box5(g)
    slots = np.array([[32, 32, 50, -1], [0, 0, 0, -1], [40, 20, 9, -1], [5, 5, 30, -1]], np.int32)   # the last is no slot of detect: inside the margin
    want_slots, want_desc = ref.describe(g, box, np.array([[32, 32, 50, -1], [0, 0, 0, -1], [40, 20, 9, -1], [0, 0, 0, -1]], np.int32))
    dirs, tables = kp._device_tables(DEV)
    tg, tb, ts = torch.from_numpy(g).to(DEV), torch.from_numpy(box).to(DEV), torch.from_numpy(slots).to(DEV)
    desc = torch.full((4, 8), -1, dtype=torch.int32, device=DEV)
    rc = _lib.load().rtgs_keypoint_describe(_lib.ptr(tg), _lib.ptr(tb), 64, 64, 4, 1, _lib.ptr(dirs), _lib.ptr(tables), _lib.ptr(ts),
                                            _lib.ptr(desc), _lib.stream(DEV))
    assert rc == 0
    torch.cuda.synchronize()
    got = ts.cpu().numpy()
    assert got[0, 3] == want_slots[0, 3] == ref.orientation_bin(*ref.moments(g, 32, 32)) and got[2, 3] == want_slots[2, 3]
    assert got[1, 3] == -1 and got[3, 3] == -1
    assert np.array_equal(words(desc)[:3], want_desc[:3]) and not desc[3].any()


def device_sets(sets):
    return {k: {"desc": torch.from_numpy(np.ascontiguousarray(v).view(np.int32)).to(DEV)} for k, v in sets.items()}


@pytest.mark.parametrize("nq,nr", [(1, 1), (5, 0), (130, 65)])
def test_match_sizes(nq, nr):
    q, r = random_desc(nq, 1), random_desc(nr, 2)
    if nr:
        r[::7] = q[:len(r[::7])]
    got, = kp.match_pairs(device_sets({"q": q, "r": r}), [("q", "r")])
    assert got.dtype == np.int32 and np.array_equal(got, ref.match(q, r))


def test_match_ties_and_the_last_bit():
    q = random_desc(3, 3)
    a = np.zeros((1, 8), np.uint32)
    b = a.copy()
    b[0, 7] = np.uint32(1) << np.uint32(31)
    sets = device_sets({"q": q[:1], "same": np.repeat(q[:1], 6, axis=0), "a": a, "bab": np.concatenate([b, a, b]), "bb": np.concatenate([b, b]),
                        "wide": np.repeat(q[1:2], 700, axis=0)})
    same, bab, bb, wide = kp.match_pairs(sets, [("q", "same"), ("a", "bab"), ("a", "bb"), ("wide", "wide")])
    assert np.array_equal(same, [[0, 0, 0]]) and np.array_equal(bab, [[1, 0, 1]]) and np.array_equal(bb, [[0, 1, 1]])
    assert np.array_equal(wide, np.tile(np.array([0, 0, 0], np.int32), (700, 1)))     # 700 equal references over three tiles: the lowest index


def test_a_batch_in_one_launch_tiles_and_repeatability(monkeypatch):
    from rtg_slam_amd import _lib
    lib = _lib.load()
    calls = [0]

    def counted(*a, _real=lib.rtgs_keypoint_match):
        calls[0] += 1
        return _real(*a)
    monkeypatch.setattr(lib, "rtgs_keypoint_match", counted)
    sizes = {"a1": 1, "b1": 1, "a2": 130, "b2": 65, "a3": 211, "b3": 300, "big": 1000}
    sets = {k: random_desc(n, 10 + i) for i, (k, n) in enumerate(sizes.items())}
    sets["b3"][5::11] = sets["a3"][:len(sets["b3"][5::11])]        # exact hits, and near hits two bits off
    sets["b2"][::3] = sets["a2"][:len(sets["b2"][::3])] ^ np.uint32(3)
    sets["big"][300:511] = sets["a3"]                              # the best lies in the second tile of 256
    sets["big"][900] = sets["a3"][7]                               # and, for one query, again in the fourth: the lower index wins
    dev = device_sets(sets)
    pairs = [("a1", "b1"), ("b1", "a1"), ("a2", "b2"), ("b2", "a2"), ("a3", "b3"), ("b3", "a3"), ("a3", "big"), ("big", "a3")]
    got = kp.match_pairs(dev, pairs)
    assert calls[0] == 1
    for (q, r), g in zip(pairs, got):
        assert g.shape == (sizes[q], 3) and np.array_equal(g, ref.match(sets[q], sets[r])), (q, r)
    assert np.array_equal(got[4][:20], brute_match(sets["a3"][:20], sets["b3"]))          # the definition against plain Python, too
    assert (got[6][:, 0] == np.arange(300, 511)).all() and (got[6][:, 1] == 0).all() and got[6][7, 2] == 0
    again = kp.match_pairs(dev, pairs)
    assert calls[0] == 2 and all(np.array_equal(x, y) for x, y in zip(got, again))


def test_relative_pose_is_the_definitions():
    """Two runs on the device are bit-equal, and equal to the definition: the same features, matches, inliers and pose."""
    fr = wide_turn_frames()
    a, b = WIDE_PAIRS[0]
    f = {}
    for k in (a, b):
        d, c, _ = fr[KEYFRAMES[k]]
        f[k] = [kp.detect_and_describe(c.to(DEV), d.to(DEV).reshape(1, CAM.H, CAM.W), K_CAM) for _ in range(2)]
        assert torch.equal(f[k][0]["desc"], f[k][1]["desc"]) and np.array_equal(f[k][0]["xyz"], f[k][1]["xyz"])
        assert np.array_equal(words(f[k][0]["desc"]), features_of(fr[KEYFRAMES[k]][2])["desc"])
    r = kp.relative_pose(f[a][0], f[b][0])
    fa, fb = features_of(fr[KEYFRAMES[a]][2]), features_of(fr[KEYFRAMES[b]][2])
    m = ref.filter_matches(ref.match(fb["desc"], fa["desc"]), ref.match(fa["desc"], fb["desc"]))
    T, mask, rms = ref.ransac_rigid(fa["xyz"][[j for _, j, _ in m]], fb["xyz"][[i for i, _, _ in m]])
    print(f"pair {a, b}: {r['keypoints_a']} / {r['keypoints_b']} keypoints, {r['matches']} matches, {r['inliers']} inliers, rms {1e3 * r['rms']:.1f} mm")
    assert r["reason"] is None and r["matches"] == len(m) and r["inliers"] == int(mask.sum()) and r["rms"] == rms
    assert np.array_equal(r["T"], T) and set(r) == {"T", "inliers", "matches", "rms", "keypoints_a", "keypoints_b", "reason"}
    strict = kp.relative_pose(f[a][0], f[b][0], kp.config(min_inliers=200))
    assert strict["T"] is None and strict["reason"] == f"{r['inliers']} inliers of {len(m)} matches, below 200"


def test_refusals():
    d, c = textured_view(view_pose(20.0))
    with pytest.raises(ValueError):
        kp.detect_and_describe(c, d.reshape(1, CAM.H, CAM.W), K_CAM)                       # CPU tensors: there is no CPU path
    with pytest.raises(ValueError):
        kp.detect_and_describe(c.to(DEV).double(), d.to(DEV), K_CAM)
    with pytest.raises(ValueError):
        kp.match_pairs({"a": {"desc": torch.zeros((3, 8), dtype=torch.int32)}}, [("a", "a")])
    with pytest.raises(ValueError):
        kp.config(cell=64)
    from rtg_slam_amd import _lib
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    assert lib.rtgs_keypoint_detect(_lib.ptr(t), _lib.ptr(t), 4, 4, 64, 20, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.stream(DEV)) == -1
    assert lib.rtgs_keypoint_detect(_lib.ptr(t), _lib.ptr(t), 4, 4, 16, 256, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.stream(DEV)) == -1
    assert lib.rtgs_keypoint_match(_lib.ptr(t), 8, _lib.ptr(t), 70000, 1, _lib.ptr(t), 8, _lib.stream(DEV)) == -1
    # a pair table that points outside the buffers is skipped, not followed: `out` keeps what it held
    tab = torch.tensor([[0, 4, 0, 1 << 20, 0], [0, 1 << 20, 0, 4, 0], [-1, 1, 0, 1, 0], [0, 2, 0, 2, 7]], dtype=torch.int32, device=DEV)
    desc = torch.zeros((8, 8), dtype=torch.int32, device=DEV)
    out = torch.full((8, 3), 77, dtype=torch.int32, device=DEV)
    assert lib.rtgs_keypoint_match(_lib.ptr(desc), 8, _lib.ptr(tab), 4, 4, _lib.ptr(out), 8, _lib.stream(DEV)) == 0
    torch.cuda.synchronize()
    assert (out == 77).all()
