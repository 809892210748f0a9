"""csrc/keypoint_pyramid.hip against tests/keypoint_pyramid_reference.py: rtgs_keypoint_pyramid, rtgs_keypoint_detect_levels and
rtgs_keypoint_describe_levels are integer arithmetic after level 0's grey value, so every comparison here is np.array_equal /
torch.equal."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import _lib
from rtg_slam_amd import keypoints as kp
from tests import keypoint_pyramid_reference as pyr
from tests import keypoint_reference as ref
from tests.test_keypoint_pyramid_cpu import features_of
from tests.test_keypoints_cpu import K_CAM, textured_view, view_pose
from tests.test_keypoints_gpu import K_SMALL, blocks_image, words
from tests.test_loop_closure_gpu import CAM, DEV

pytestmark = pytest.mark.gpu
F32 = np.float32


def run_levels(color, depth, table, cell=16, threshold=20, oriented=True):
    """The three entry points over a level table of the caller's -> the packed g8, depth, box5 planes, the slots and the
    descriptors as numpy arrays."""
    table = np.ascontiguousarray(table, dtype=np.int32)
    total = int(table[-1, 0] + table[-1, 1] * table[-1, 2])
    cells = sum((-(-int(h) // cell)) * (-(-int(w) // cell)) for _, h, w, _, _ in table)
    c, z = torch.from_numpy(np.ascontiguousarray(color)).to(DEV), torch.from_numpy(np.ascontiguousarray(depth)).to(DEV)
    g8 = torch.full((total,), 7, dtype=torch.uint8, device=DEV)
    dl = torch.full((total,), -7.0, dtype=torch.float32, device=DEV)
    box = torch.full((total,), -7, dtype=torch.int32, device=DEV)
    slots = torch.full((cells, 4), -7, dtype=torch.int32, device=DEV)
    desc = torch.full((cells, 8), -7, dtype=torch.int32, device=DEV)
    dirs, tables = kp._device_tables(DEV)
    lib, lv, n, st = _lib.load(), table.ctypes.data, len(table), _lib.stream(DEV)
    assert lib.rtgs_keypoint_pyramid(_lib.ptr(c), _lib.ptr(z), lv, n, total, _lib.ptr(g8), _lib.ptr(dl), st) == 0
    assert lib.rtgs_keypoint_detect_levels(_lib.ptr(g8), _lib.ptr(dl), lv, n, total, cell, threshold, _lib.ptr(box), _lib.ptr(slots), st) == 0
    assert lib.rtgs_keypoint_describe_levels(_lib.ptr(g8), _lib.ptr(box), lv, n, total, cell, int(oriented), _lib.ptr(dirs), _lib.ptr(tables),
                                             _lib.ptr(slots), _lib.ptr(desc), st) == 0
    torch.cuda.synchronize()
    return {"g8": g8.cpu().numpy(), "depth": dl.cpu().numpy(), "box5": box.cpu().numpy(), "slots": slots.cpu().numpy(), "slot_desc": words(desc)}


def assert_levels_equal(got, want):
    t = want["table"]
    assert np.array_equal(got["g8"], pyr.packed(want["g8"], t, np.uint8))
    assert np.array_equal(got["depth"].view(np.uint32), pyr.packed(want["depth"], t, F32).view(np.uint32))      # bits: NaN and inf too
    assert np.array_equal(got["box5"], pyr.packed(want["box5"], t, np.int32))
    assert np.array_equal(got["slots"], want["slots"])
    assert np.array_equal(got["slot_desc"], want["slot_desc"])


@pytest.mark.parametrize("H,W,levels,over", [(35, 50, 5, dict(cell=8)), (33, 47, 5, dict(cell=8)), (100, 131, 5, dict(cell=8, threshold=10)),
                                             (100, 131, 3, dict(cell=28)), (97, 150, 4, dict(cell=16, oriented=False)), (48, 48, 2, {}),
                                             (49, 97, 5, dict(cell=32))])
def test_the_kernels_match_the_definition_on_odd_sizes_holes_and_nan(H, W, levels, over):
    """Sizes that are no multiple of the 48-pixel tile, of 2, 3 or the cell; a depth with holes, NaN, inf and negative values; every
    level of the ladder whatever its size (a table without the drop rule)."""
    color, depth = blocks_image(H, W, H + W)
    color[:, 3, 5] = np.nan                                         # a NaN colour is grey 0, and goes into the levels as 0
    table = pyr.level_table(H, W, levels)
    cfg = kp.config(**over)
    want = pyr.detect_and_describe(color, depth, cfg.threshold, cfg.cell, cfg.oriented, table=table)
    got = run_levels(color, depth, table, cfg.cell, cfg.threshold, cfg.oriented)
    print(f"{W} x {H}, {len(table)} levels {over}: {len(want['x'])} keypoints on levels {sorted(set(want['level'].tolist()))}")
    assert len(table) == levels and np.isnan(want["depth"][min(1, levels - 1)]).any()
    assert_levels_equal(got, want)


@pytest.mark.parametrize("levels", [1, 3, 5])
def test_a_textured_view_matches_the_definition(levels):
    T = view_pose(20.0)
    d, c = textured_view(T)
    want = features_of(T, levels)
    cfg = kp.config(levels=levels)
    f = kp.detect_and_describe(c.to(DEV), d.to(DEV).reshape(1, CAM.H, CAM.W), K_CAM, cfg, keep_planes=True)
    print(f"320 x 240, {levels} levels: {len(want['x'])} keypoints, per level {np.bincount(want['level']).tolist()}")
    for k in ("x", "y", "score", "bin"):
        assert f[k].dtype == np.int32 and np.array_equal(f[k], want[k]), k
    assert np.array_equal(words(f["desc"]).reshape(-1, 8), want["desc"].reshape(-1, 8))
    assert f["xyz"].dtype == np.float64 and np.array_equal(f["xyz"], want["xyz"])
    if levels == 1:                                                 # today's calls, today's dict
        assert set(f) == {"x", "y", "score", "bin", "desc", "xyz", "g8", "box5", "slots", "slot_desc"}
        return
    assert set(f) == {"x", "y", "score", "bin", "desc", "xyz", "level", "x0", "y0", "levels_used", "g8", "depth_levels", "box5", "slots",
                      "slot_desc", "table"}
    assert f["levels_used"] == levels and np.array_equal(f["table"], want["table"]) and len(set(want["level"].tolist())) == levels
    assert np.array_equal(f["level"], want["level"]) and np.array_equal(f["x0"], want["x0"]) and np.array_equal(f["y0"], want["y0"])
    got = {"g8": f["g8"].cpu().numpy(), "depth": f["depth_levels"].cpu().numpy(), "box5": f["box5"].cpu().numpy(), "slots": f["slots"].cpu().numpy(),
           "slot_desc": words(f["slot_desc"])}
    assert_levels_equal(got, want)


def test_a_dropped_level_and_three_launches_whatever_the_levels(monkeypatch):
    lib = _lib.load()
    names = ("rtgs_keypoint_pyramid", "rtgs_keypoint_detect_levels", "rtgs_keypoint_describe_levels", "rtgs_keypoint_detect", "rtgs_keypoint_describe")
    calls = {n: 0 for n in names}
    for name in names:
        def counted(*a, _real=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    color, depth = blocks_image(120, 160, 9)
    c, z = torch.from_numpy(color).to(DEV), torch.from_numpy(depth).to(DEV)[None]
    f = kp.detect_and_describe(c, z, K_SMALL, kp.config(levels=5))
    assert calls == {"rtgs_keypoint_pyramid": 1, "rtgs_keypoint_detect_levels": 1, "rtgs_keypoint_describe_levels": 1, "rtgs_keypoint_detect": 0,
                     "rtgs_keypoint_describe": 0}
    want = pyr.detect_and_describe(color, depth, levels=5)
    assert f["levels_used"] == want["levels_used"] == 3             # level 3 would be 53 x 40: no cell of 16 inside the margin
    assert np.array_equal(f["level"], want["level"]) and np.array_equal(words(f["desc"]).reshape(-1, 8), want["desc"].reshape(-1, 8))
    assert np.array_equal(f["xyz"], pyr.backproject(want, K_SMALL))
    one = kp.detect_and_describe(c, z, K_SMALL, kp.config(levels=1))
    assert calls["rtgs_keypoint_pyramid"] == 1 and calls["rtgs_keypoint_detect"] == 1 and calls["rtgs_keypoint_describe"] == 1
    assert "level" not in one and "levels_used" not in one


def test_one_level_through_the_new_entry_points_is_the_old_entry_points_output_and_two_runs_are_bit_equal():
    color, depth = blocks_image(83, 101, 4)
    old = kp.detect_and_describe(torch.from_numpy(color).to(DEV), torch.from_numpy(depth).to(DEV)[None], K_SMALL, keep_planes=True)
    new = run_levels(color, depth, pyr.level_table(83, 101, 1))
    assert np.array_equal(new["g8"], old["g8"].cpu().numpy().reshape(-1)) and np.array_equal(new["box5"], old["box5"].cpu().numpy().reshape(-1))
    assert np.array_equal(new["slots"], old["slots"].cpu().numpy()) and np.array_equal(new["slot_desc"], words(old["slot_desc"]))
    assert (new["slots"][:, 2] > 0).sum() >= 2
    table = pyr.level_table(83, 101, 5)
    a, b = run_levels(color, depth, table, 8), run_levels(color, depth, table, 8)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_bad_arguments_return_minus_one_without_a_launch():
    lib, st = _lib.load(), _lib.stream(DEV)
    t = torch.full((4096,), 77, dtype=torch.int32, device=DEV)
    p = _lib.ptr(t)
    good = pyr.level_table(35, 50, 3)
    total = int(good[-1, 0] + good[-1, 1] * good[-1, 2])

    def all_three(table, n, total, cell=8, threshold=20):
        lv = np.ascontiguousarray(table, dtype=np.int32).ctypes.data
        return (lib.rtgs_keypoint_pyramid(p, p, lv, n, total, p, p, st), lib.rtgs_keypoint_detect_levels(p, p, lv, n, total, cell, threshold, p, p, st),
                lib.rtgs_keypoint_describe_levels(p, p, lv, n, total, cell, 1, p, p, p, p, st))
    bad = []
    for row, col, value in ((1, 1, 23), (1, 2, 33), (2, 1, 18), (1, 3, 2), (2, 4, 2), (0, 0, -1), (1, 0, 5), (2, 0, total)):
        t2 = good.copy()
        t2[row, col] = value                                        # not the ladder's size or scale, a negative offset, an overlap, past the end
        bad.append((t2, 3, total))
    bad += [(good, 0, total), (good, 6, total), (good, 3, total - 1), (good, 3, 0), (good, 3, 1 << 31)]
    for table, n, tot in bad:
        assert all_three(table, n, tot) == (-1, -1, -1), (table.tolist(), n, tot)
    lv = good.ctypes.data
    assert lib.rtgs_keypoint_pyramid(None, p, lv, 3, total, p, p, st) == -1 and lib.rtgs_keypoint_pyramid(p, p, None, 3, total, p, p, st) == -1
    assert lib.rtgs_keypoint_detect_levels(p, p, lv, 3, total, 7, 20, p, p, st) == -1
    assert lib.rtgs_keypoint_detect_levels(p, p, lv, 3, total, 8, 256, p, p, st) == -1
    assert lib.rtgs_keypoint_detect_levels(p, p, lv, 3, total, 8, 20, None, p, st) == -1
    assert lib.rtgs_keypoint_describe_levels(p, p, lv, 3, total, 33, 1, p, p, p, p, st) == -1
    assert lib.rtgs_keypoint_describe_levels(p, p, lv, 3, total, 8, 1, p, p, p, None, st) == -1
    torch.cuda.synchronize()
    assert (t == 77).all()                                          # nothing was launched
    with pytest.raises(ValueError):
        kp.config(levels=0)
    with pytest.raises(ValueError):
        kp.config(levels=6)
    with pytest.raises(ValueError):
        kp.config(levels=2.5)
