"""The definition of the RGB-D pose refinement (tests/rgbd_align_reference.py) on its own: what it recovers where geometry
cannot, that its geometric part is the ICP tracker's, that it leaves what it cannot observe alone, and its gates.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import icp_oracle as io
from rtg_slam_amd import synth
from tests import rgbd_align_reference as ref

DIST, COS = 0.1, float(np.cos(np.deg2rad(20.0)))


def single(s):
    return [[s[k]] for k in ("v_src", "n_src", "i_src", "v_tgt", "n_tgt", "i_tgt")]


def sums(s, pose=None, photo_weight=0.25, huber=0.05):
    return ref.accumulate(s["v_src"], s["n_src"], s["i_src"], s["v_tgt"], s["n_tgt"], s["i_tgt"], s["K"],
                          np.eye(4) if pose is None else pose, DIST, COS, photo_weight, huber)


def test_flat_textured_wall_is_recovered_where_geometry_has_rank_three():
    """Plane z = 2 m at 80 x 60, fx = fy = 70, displaced by xi = (0.004, -0.003, 0.006 rad; 20, -15, 10 mm).  The geometric H
    has exactly three eigenvalues under 1e-9 lambda_max (this file's float32 definition: 0, 0, 0, 1025, 1853, 4524).  refine
    from the identity at a single level must leave at most 5 % of the initial translation error; the reference itself goes
    from 26.93 mm to 0.20 mm and stops, converged, after 4 iterations (a float64 prototype: 26.9 mm to 0.04 mm in 12)."""
    s = ref.wall_pair()
    A, _ = ref.mrr.normal_matrix(sums(s, photo_weight=0.0)[:27])
    lam = np.linalg.eigvalsh(A)
    assert int((lam <= 1e-9 * lam[-1]).sum()) == 3, lam
    T, rep = ref.refine(np.eye(4), *single(s), s["K"], [1.0], iters=[12], distance_threshold=DIST, cos_threshold=COS)
    before = np.linalg.norm(s["truth"][:3, 3])
    after = np.linalg.norm(T[:3, 3] - s["truth"][:3, 3])
    print(f"translation error {1e3 * before:.3f} mm -> {1e3 * after:.3f} mm in {rep['iterations']} iterations, rank {rep['rank']}")
    assert 0.026 < before < 0.028
    assert after <= 0.05 * before
    assert rep["rank"][-1] == 6


def test_geometric_part_is_the_icp_oracles():
    """photo_weight = 0: the 27 values of H and b against oracle.icp_oracle.residuals_jacobian + normal_equations on doubles
    (exact_sums), to 1e-5 of the largest |H| entry - float32 products against products of the widened factors differ by
    2^-24 relative, a hundredfold margin - and the geometric count against the oracle's valid.sum().  Relief room, a moved
    pose, so that all 27 are non-zero."""
    cam = synth.CameraSpec(60, 80, 70.0, 70.0, 39.5, 29.5)
    K = torch.tensor([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=torch.float32)
    poses = synth.trajectory(2, seed=9)
    base = synth.look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3)
    v0 = io.vertex_map(synth.box_room_depth(cam, base @ poses[0]), K)
    v1 = io.vertex_map(synth.box_room_depth(cam, base @ poses[1]), K)
    n0, n1 = io.normal_map(v0), io.normal_map(v1)
    pose = synth.se3_exp(torch.tensor([0.002, -0.001, 0.003, 0.004, -0.002, 0.003])).float()
    res, J, valid = io.residuals_jacobian(v1, v0, n1, n0, pose, K, DIST, COS)
    JtJ, Jtr = io.normal_equations(J.double(), res.double())
    grey = np.zeros((cam.H, cam.W), np.float32)
    out = ref.accumulate(v1.numpy(), n1.numpy(), grey, v0.numpy(), n0.numpy(), grey, K.numpy(), pose.numpy(), DIST, COS, 0.0, 0.05)
    A, b = ref.mrr.normal_matrix(out[:27])
    scale = float(JtJ.abs().max())
    assert int(valid.sum()) > 1000
    assert int(out[28]) == int(valid.sum())
    assert np.abs(A - JtJ.numpy()).max() <= 1e-5 * scale
    assert np.abs(b - Jtr.numpy()).max() <= 1e-5 * scale


def test_textureless_flat_wall_leaves_what_it_cannot_observe_at_the_initial_guess():
    s = ref.wall_pair(textured=False)
    init = ref.se3_exp(np.array([0.001, 0.002, -0.003, 0.007, -0.004, 0.002]))
    T, rep = ref.refine(init, *single(s), s["K"], [1.0], iters=[5], distance_threshold=DIST, cos_threshold=COS)
    assert np.isfinite(T).all()
    assert rep["rank"] and all(r == 3 for r in rep["rank"])
    # The wall's normal is the target's z axis: x, y translation and the rotation about z are not observable.  No twist that was
    # applied has a component there: those rows and columns of H are exactly 0, so the kept eigenvectors' entries are 0 to
    # eigh's accuracy, 2.2e-16, times twists under 0.05
    X = np.array(rep["twists"])
    assert np.abs(X).max() < 0.05
    assert np.abs(X[:, [2, 3, 4]]).max() <= 2.2e-16 * 0.05
    # ... so the whole update, delta = T init^-1 = prod exp(x_k), moves in the plane and turns about the normal only by the
    # second-order products of the tilts and the step along the normal: bounded by (sum |w_k|) (sum |v_k|) and (sum |w_k|)^2,
    # two orders under the 25 mm and 6 mrad the view cannot see
    delta = T @ np.linalg.inv(init)
    sw, sv = np.linalg.norm(X[:, :3], axis=1).sum(), np.linalg.norm(X[:, 3:], axis=1).sum()
    assert sw * sv < 2e-4 and sw * sw < 1e-4
    assert np.abs(delta[:2, 3]).max() <= sw * sv
    assert abs(delta[1, 0] - delta[0, 1]) / 2 <= sw * sw
    # and what it can observe is found: distance along the normal and the tilt
    assert abs(T[2, 3] - s["truth"][2, 3]) < 2e-4
    assert np.abs(T[2, :2] - s["truth"][2, :2]).max() < 2e-4


def test_relief_room_is_no_farther_from_the_truth_than_icp():
    """The pair: synth.trajectory(2, seed=4) on look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3) at 160 x 120, f = 130,
    box_room_depth's default relief and box_room_color, clean and with tum_noise(seeds 1, 2); the start is the ICP oracle's
    pose (exact_sums).  The reference: clean 0.180 mm -> 0.092 mm, noisy 10.35 mm -> 9.28 mm."""
    cam = synth.CameraSpec(120, 160, 130.0, 130.0, 79.5, 59.5)
    K = torch.tensor([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=torch.float32)
    poses = synth.trajectory(2, seed=4)
    base = synth.look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3)
    c0, c1 = base @ poses[0], base @ poses[1]
    truth = (torch.linalg.inv(c0) @ c1).numpy()
    for noisy in (False, True):
        d0, d1 = synth.box_room_depth(cam, c0), synth.box_room_depth(cam, c1)
        i0 = ref.intensity_pyramid(synth.box_room_color(cam, c0, d0).numpy(), 3)
        i1 = ref.intensity_pyramid(synth.box_room_color(cam, c1, d1).numpy(), 3)
        if noisy:
            d0, d1 = synth.tum_noise(d0, 1), synth.tum_noise(d1, 2)
        vp0, vp1 = io.vertex_pyramid(d0, K, 3), io.vertex_pyramid(d1, K, 3)
        np0, np1 = io.normal_pyramid(vp0), io.normal_pyramid(vp1)
        icp_pose, _, _ = io.track(vp1, np1, vp0, np0, K, exact_sums=True)
        arr = lambda L: [x.numpy() for x in L]
        T, rep = ref.refine(icp_pose.numpy(), arr(vp1), arr(np1), i1, arr(vp0), arr(np0), i0, K.numpy(), [0.25, 0.5, 1.0],
                            distance_threshold=DIST, cos_threshold=COS)
        e_icp = np.linalg.norm(icp_pose.numpy().astype(np.float64)[:3, 3] - truth[:3, 3])
        e_ref = np.linalg.norm(T[:3, 3] - truth[:3, 3])
        print(f"noisy {noisy}: icp {1e3 * e_icp:.3f} mm, refined {1e3 * e_ref:.3f} mm, iterations {rep['iterations']}")
        assert rep["rank"][-1] == 6
        assert e_ref <= e_icp


def one_pixel_case(src_intensity, u_shift=0.0, depth=2.0):
    """A 6 x 5 fronto-parallel plane with a horizontal intensity ramp in the target and a constant source; only the source
    pixel (2, 2) has depth."""
    H, W = 5, 6
    K = np.array([[4.0, 0, 2.5], [0, 4.0, 2.0], [0, 0, 1]], np.float32)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    v_t = np.stack([(xs - K[0, 2]) / K[0, 0] * 2, (ys - K[1, 2]) / K[1, 1] * 2, np.full((H, W), 2, np.float32)], -1).astype(np.float32)
    n = np.broadcast_to(np.array([0, 0, -1], np.float32), (H, W, 3)).copy()
    i_t = (0.1 * xs).astype(np.float32)
    v_s = np.zeros((H, W, 3), np.float32)
    v_s[2, 2] = v_t[2, 2] * np.float32(depth / 2.0) if np.isfinite(depth) else np.float32(np.nan)
    v_s[2, 2, 0] += np.float32(u_shift * 2.0 / 4.0) * np.float32(depth / 2.0 if np.isfinite(depth) else 1.0)
    i_s = np.full((H, W), src_intensity, np.float32)
    return v_s, n, i_s, v_t, n, i_t, K


def test_huber_weight_and_the_edges_of_the_gates():
    huber = 0.05
    # target intensity at the pixel's own place is 0.2 (+ 0.01 for the 0.1 px shift that keeps u off the lattice)
    for src, expect in ((0.2, 1.0), (0.0, None)):
        case = one_pixel_case(src, u_shift=0.1)
        t = ref.pixel_terms(*case, np.eye(4), DIST, COS, 0.25, huber)
        i = 2 * 6 + 2
        assert t["photo"][i] and t["geo"][i] and t["photo"].sum() == 1
        r = abs(float(t["rI"][i]))
        if expect is None:
            assert r > huber and t["w"][i] == np.float32(huber) / np.abs(t["rI"][i]) and t["w"][i] < 1
        else:
            assert r <= huber and t["w"][i] == 1
        out = ref.accumulate(*case, np.eye(4), DIST, COS, 0.25, huber)
        assert out[30] == 1 and out[28] == 1
        assert out[29] == float(t["w"][i]) * (float(t["rI"][i]) * float(t["rI"][i]))
    # u exactly W - 1: shift the pixel three columns to the right, onto the last column
    case = one_pixel_case(0.0, u_shift=3.0)
    t = ref.pixel_terms(*case, np.eye(4), DIST, COS, 0.25, huber)
    assert t["u"][2 * 6 + 2] == np.float32(5.0)
    out = ref.accumulate(*case, np.eye(4), DIST, COS, 0.25, huber)
    assert np.array_equal(out, np.zeros(31)) and not np.signbit(out).any()
    # a NaN depth
    case = one_pixel_case(0.0, depth=float("nan"))
    assert np.isnan(case[0][2, 2]).all()
    out = ref.accumulate(*case, np.eye(4), DIST, COS, 0.25, huber)
    assert np.array_equal(out, np.zeros(31)) and not np.signbit(out).any()


def test_pyramid_sizes_and_values():
    rng = np.random.default_rng(0)
    c = rng.random((3, 61, 83)).astype(np.float32)
    pyr = ref.intensity_pyramid(c, 3)
    assert [p.shape for p in pyr] == [(15, 20), (30, 41), (61, 83)]
    g = pyr[2]
    assert g[7, 9] == np.float32(np.float32(np.float32(0.299) * c[0, 7, 9] + np.float32(0.587) * c[1, 7, 9]) + np.float32(0.114) * c[2, 7, 9])
    assert pyr[1][3, 4] == np.float32(np.float32(np.float32(g[6, 8] + g[6, 9]) + np.float32(g[7, 8] + g[7, 9])) * np.float32(0.25))
