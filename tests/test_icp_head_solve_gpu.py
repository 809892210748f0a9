"""The tracker's head-solve chain (launch k+1 sums launch k's partial rows, solves and steps the pose at its head; icp_p2p
does so for the last iteration and writes the caller's pose) against the last-arriver chain it replaces
(RTGS_ICP_FLAG_LAST_ARRIVER): same arithmetic in the same order, so the 16 pose floats and the 4 stats must be EQUAL, bit
for bit, on every input.  Shapes are the smallest at which each thing can go wrong: one workgroup per level (32x32), a
pixel count that is no multiple of four at every level (101x135: 13635 / 3350 / 825 pixels), and 16 / 64 / 256 workgroups
(512x512) - the grid at which a fast workgroup of a launch writes its row, and workgroup 0 the pose, while slow ones still
read the previous launch's: the two hazards the alternating row buffers and pose slots remove."""
import math

import pytest
import torch

from rtg_slam_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COS_THR = math.cos(math.radians(20.0))          # the reference's thresholds (icp_distance_threshold 0.1, 20 degrees, 1e-4)
DIST_THR, DAMPING = 0.1, 1e-4
DS = [0.25, 0.5, 1.0]
SHAPES = {"one_wg": (32, 32), "ragged": (101, 135), "wg256": (512, 512)}
_cache = {}


def scene(name, empty_current=False):
    """(vertex_src, normal_src, vertex_tgt, normal_tgt, K) pyramids of two box-room frames, built once per shape."""
    key = (name, empty_current)
    if key not in _cache:
        from rtg_slam_amd import icp
        H, W = SHAPES[name]
        cam = synth.CameraSpec(H, W, 0.5 * W, 0.5 * W, (W - 1) / 2, (H - 1) / 2)
        poses = synth.trajectory(2, seed=9)
        base = synth.look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3)
        d0 = synth.box_room_depth(cam, base @ poses[0])
        d1 = torch.zeros_like(d0) if empty_current else synth.box_room_depth(cam, base @ poses[1])
        K = torch.tensor([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=torch.float32, device=DEV)
        v0, n0 = icp.build_pyramids(d0.to(DEV), K, 3)
        v1, n1 = icp.build_pyramids(d1.to(DEV), K, 3)
        _cache[key] = (v1, n1, v0, n0, K)
    return _cache[key]


def given_pose():
    return synth.se3_exp(torch.tensor([0.004, -0.003, 0.002, 0.01, -0.008, 0.006])).float()


def track(s, iters, pose0=None, f32_solve=False, last_arriver=False):
    from rtg_slam_amd import icp
    return icp.icp_track(s[0], s[1], s[2], s[3], s[4], DS, iters, DIST_THR, COS_THR, DAMPING, pose0=pose0,
                         f32_solve=f32_solve, last_arriver=last_arriver)


def both(s, iters, pose0=None, f32_solve=False):
    new = track(s, iters, pose0, f32_solve).cpu()
    old = track(s, iters, pose0, f32_solve, last_arriver=True).cpu()
    print("new", new.tolist(), "\nold", old.tolist())
    return new, old


@pytest.mark.parametrize("f32_solve", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("start", ["identity", "given"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forms_agree(shape, start, f32_solve):
    new, old = both(scene(shape), [5, 5, 5], None if start == "identity" else given_pose(), f32_solve)
    assert torch.equal(new, old)
    assert torch.isfinite(new).all() and float(new[19]) == 0.0
    if shape != "one_wg":                        # 8x8 pixels at the coarsest level are not asked to give a usable system
        assert float(new[18]) == 0.0 and float(new[16]) > 0.0      # two frames 2 cm apart do correspond: real solves ran


@pytest.mark.parametrize("start", ["identity", "given"])
@pytest.mark.parametrize("iters", [[0, 5, 5], [5, 0, 5], [5, 5, 0], [0, 0, 0]], ids=["055", "505", "550", "000"])
@pytest.mark.parametrize("shape", ["ragged", "wg256"])
def test_iteration_patterns(shape, iters, start):
    """A level change with no launch in between (the head is told the rows, the 1 / pixels of the launch it consumes, not
    of its own level), and the path without any launch."""
    pose0 = None if start == "identity" else given_pose()
    new, old = both(scene(shape), iters, pose0)
    assert torch.equal(new, old)
    if iters == [0, 0, 0]:
        assert torch.equal(new[:16].reshape(4, 4), torch.eye(4) if pose0 is None else pose0)


@pytest.mark.parametrize("start", ["identity", "given"])
@pytest.mark.parametrize("shape", ["ragged", "wg256"])
def test_frame_without_correspondences(shape, start):
    """Every one of the 15 systems is singular: both forms count 15 skipped steps and leave the pose as it was."""
    pose0 = None if start == "identity" else given_pose()
    new, old = both(scene(shape, empty_current=True), [5, 5, 5], pose0)
    assert torch.equal(new, old)
    assert float(new[18]) == 15.0 and float(new[16]) == 0.0
    assert torch.equal(new[:16].reshape(4, 4), torch.eye(4) if pose0 is None else pose0)


def test_hundred_tracks_back_to_back():
    """100 tracks on one scratch with no synchronisation between them: the alternating buffers start over every track."""
    s = scene("wg256")
    outs = [track(s, [5, 5, 5]) for _ in range(100)]
    torch.cuda.synchronize()
    first = outs[0].cpu()
    assert torch.equal(first, track(s, [5, 5, 5], last_arriver=True).cpu())
    bad = [i for i, o in enumerate(outs) if not torch.equal(o.cpu(), first)]
    assert not bad, bad


@pytest.mark.parametrize("order", ["new_old", "old_new"])
def test_forms_alternate_on_one_scratch(order):
    """Either form leaves the scratch armed for the other (the ticket is 0 after icp_p2p's last arriver in both)."""
    s = scene("wg256")
    flags = [False, True, False, True] if order == "new_old" else [True, False, True, False]
    outs = [track(s, [5, 5, 5], last_arriver=f) for f in flags]
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o.cpu(), outs[0].cpu())
