"""The tracker's residual and point-to-plane kernels (one quad of source pixels per lane, target vertex and normal gathered
in one round trip, fused multiply-adds in the 27 sums, pose read ahead of the last arriver's solve) at the two shipped
frame sizes, on clean and noisy depth: exact valid counts, sums against float64, the 15-iteration pose, the loss, and the
last arriver re-arming the ticket."""
import math

import numpy as np
import pytest
import torch

from oracle import icp_oracle as io
from rtg_slam_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COS_THR = math.cos(math.radians(20.0))
CASES = [(synth.REPLICA, False), (synth.REPLICA, True), (synth.TUM_FR1, False), (synth.TUM_FR1, True)]
IDS = ["replica_clean", "replica_noisy", "tum_clean", "tum_noisy"]


def frames(cam, noise):
    poses = synth.trajectory(2, seed=9)
    base = synth.look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3)
    d0 = synth.box_room_depth(cam, base @ poses[0])
    d1 = synth.box_room_depth(cam, base @ poses[1])
    if noise:
        d0, d1 = synth.tum_noise(d0, 1), synth.tum_noise(d1, 2)
    K = torch.tensor([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=torch.float32)
    return d0, d1, K


def pyramids(d0, d1, K):
    from rtg_slam_amd import icp
    hv0, hn0 = icp.build_pyramids(d0.to(DEV), K.to(DEV), 3)
    hv1, hn1 = icp.build_pyramids(d1.to(DEV), K.to(DEV), 3)
    return hv0, hn0, hv1, hn1


@pytest.mark.parametrize("cam,noise", CASES, ids=IDS)
def test_step_counts_and_sums(cam, noise):
    """At the identity pose (the first step of a track; p = v exactly on both sides) every level's valid count is the
    oracle's, and the 27 sums are the float64 sums of the oracle's per-pixel terms to 1e-5 of their largest entry."""
    from rtg_slam_amd import icp
    d0, d1, K = frames(cam, noise)
    hv0, hn0, hv1, hn1 = pyramids(d0, d1, K)
    pose = torch.eye(4)
    for l, ds in enumerate([0.25, 0.5, 1.0]):
        Kl = K * ds
        Kl[2, 2] = 1.0
        res, J, valid = io.residuals_jacobian(hv1[l].cpu(), hv0[l].cpu(), hn1[l].cpu(), hn0[l].cpu(), pose, Kl, 0.1, COS_THR)
        JtJ, Jtr, nv = icp.icp_step(hv1[l], hn1[l], hv0[l], hn0[l], Kl, pose, 0.1, COS_THR)
        assert int(nv.item()) == int(valid.sum()), (l, int(nv.item()), int(valid.sum()))
        J64, r64 = J.double(), res.double()
        JtJ64, Jtr64 = J64.t() @ J64, J64.t() @ r64
        assert float((JtJ.cpu().double() - JtJ64).abs().max()) <= 1e-5 * float(JtJ64.abs().max()), l
        assert float((Jtr.cpu().double() - Jtr64).abs().max()) <= 1e-5 * float(Jtr64.abs().max()) + 1e-9, l


@pytest.mark.parametrize("cam,noise", CASES, ids=IDS)
def test_track_pose_loss_and_ticket(cam, noise):
    """Two tracks back to back on one scratch give the same result (the last arriver of every launch re-armed the ticket);
    the loss is the float64 sum of the per-pixel terms at the final pose; on clean depth the 15-iteration pose is the
    exact-sum oracle's to 1e-5."""
    from rtg_slam_amd import icp
    d0, d1, K = frames(cam, noise)
    hv0, hn0, hv1, hn1 = pyramids(d0, d1, K)
    run = lambda: icp.icp_track(hv1, hn1, hv0, hn0, K, [0.25, 0.5, 1.0], [5, 5, 5], 0.1, COS_THR, 1e-4).cpu()
    a = run()
    b = run()
    torch.cuda.synchronize()
    assert torch.equal(a, b), (a - b).abs().max()
    assert float(a[18]) == 0.0 and float(a[19]) == 0.0
    P = a[:16].reshape(4, 4)
    # point2plane_loss in the kernel's float32 op order, summed in float64
    v1, v0, n0 = hv1[2].cpu().reshape(-1, 3), hv0[2].cpu().reshape(-1, 3), hn0[2].cpu().reshape(-1, 3)
    p = [(v1[:, 0] * P[r, 0] + v1[:, 1] * P[r, 1] + v1[:, 2] * P[r, 2]) + P[r, 3] for r in range(3)]
    lp = (p[0] - v0[:, 0]) * n0[:, 0] + (p[1] - v0[:, 1]) * n0[:, 1] + (p[2] - v0[:, 2]) * n0[:, 2]
    loss64 = float((lp.double() ** 2).sum() / v1.shape[0])
    assert abs(float(a[17]) - loss64) <= 1e-5 * loss64, (float(a[17]), loss64)
    if not noise:
        vp0 = io.vertex_pyramid(d0, K.clone(), 3); np0 = io.normal_pyramid(vp0)
        vp1 = io.vertex_pyramid(d1, K.clone(), 3); np1 = io.normal_pyramid(vp1)
        pose_x, _, _ = io.track(vp1, np1, vp0, np0, K.clone(), exact_sums=True)
        err = float((P - pose_x).abs().max())
        assert err < 1e-5, err
