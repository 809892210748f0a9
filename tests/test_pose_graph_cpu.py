"""rtg_slam_amd/pose_graph.py and rgbd_align.se3_log on the host: no device."""
import numpy as np
import pytest

from rtg_slam_amd import pose_graph as pg
from rtg_slam_amd.rgbd_align import se3_exp, se3_log

RING = 24
DRIFT = np.array([0.0, np.deg2rad(0.03), 0.0, 0.0015, 0.0, 0.0])          # per node: 0.03 degrees about y, 1.5 mm along x


def ring_truth(n=RING, radius=1.0, wobble=0.1):
    """Cameras on a circle in the x-z plane, each turned with its position (yaw about y), at a height that varies."""
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        T = se3_exp([0.0, a, 0.0, 0.0, 0.0, 0.0])
        T[:3, 3] = (radius * np.sin(a), wobble * np.sin(3 * a), radius * (1 - np.cos(a)))
        out.append(T)
    return np.array(out)


def ring_case(w_rot=1.0, w_trans=1.0):
    """-> (true poses, drifted poses, edges): every odometry edge carries the same small error in its own frame, the loop edge
    last -> first is the truth.  A general graph for the tests of the optimiser itself."""
    truth = ring_truth()
    D = se3_exp(DRIFT)
    drifted, edges = [truth[0]], []
    for k in range(1, RING):
        Z = pg.inverse(truth[k - 1]) @ truth[k] @ D
        edges.append((k - 1, k, Z, w_rot, w_trans))
        drifted.append(drifted[-1] @ Z)
    edges.append((RING - 1, 0, pg.inverse(truth[-1]) @ truth[0], w_rot, w_trans, True))
    return truth, np.array(drifted), edges


def trans_err(a, b):
    return np.linalg.norm(a[:, :3, 3] - b[:, :3, 3], axis=1)


def test_log_inverts_exp():
    rng = np.random.default_rng(3)
    for scale in (1e-10, 1e-4, 0.3, 2.0, 3.1):
        for _ in range(20):
            x = rng.normal(size=6)
            x[:3] *= scale / np.linalg.norm(x[:3])
            T = se3_exp(x)
            assert np.abs(se3_log(T) - x).max() < 1e-9, (scale, x)
            assert np.abs(se3_exp(se3_log(T)) - T).max() < 1e-12
    assert np.array_equal(se3_log(np.eye(4)), np.zeros(6))
    half_turn = se3_exp([0.0, np.pi, 0.0, 0.1, 0.2, 0.3])
    assert np.abs(se3_exp(se3_log(half_turn)) - half_turn).max() < 1e-9


def test_right_jacobian_by_differences():
    rng = np.random.default_rng(5)
    r = rng.normal(size=6) * 0.4
    J = pg.right_jacobian_inverse(r)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        num = (se3_log(se3_exp(r) @ se3_exp(d)) - se3_log(se3_exp(r) @ se3_exp(-d))) / (2 * h)
        assert np.abs(num - J[:, k]).max() < 1e-8


def test_consistent_graph_returns_its_input_with_zero_cost():
    truth = ring_truth()
    edges = [(k, (k + 1) % RING, pg.inverse(truth[k]) @ truth[(k + 1) % RING], 2.0, 3.0) for k in range(RING)]
    out, rep = pg.optimize(truth, edges)
    assert np.abs(out - truth).max() < 1e-12
    assert rep["cost_before"] < 1e-24 and rep["cost_after"] < 1e-24 and rep["last_update"] < 1e-10


def linear_drift_case(radius, loop_weight):
    """The drifted pose of node k is exp(k DRIFT) T_k - an error that grows linearly along the trajectory, D_0 = I -, the
    odometry edges are read off the drifted poses, and the one loop edge last -> first is the truth, weighted as what it is."""
    truth = ring_truth(radius=radius, wobble=0.0)
    drifted = np.array([se3_exp(k * DRIFT) @ truth[k] for k in range(RING)])
    edges = [(k - 1, k, pg.inverse(drifted[k - 1]) @ drifted[k], 1.0, 1.0) for k in range(1, RING)]
    edges.append((RING - 1, 0, pg.inverse(truth[-1]) @ truth[0], loop_weight, loop_weight, True))
    return truth, drifted, edges


def errors(poses, truth):
    rot = max(np.linalg.norm(se3_log(pg.inverse(t) @ p)[:3]) for t, p in zip(truth, poses))
    return trans_err(poses, truth), rot


def test_ring_drift_is_removed():
    """24 headings round a full circle from one place (the loop tests/test_loop_closure_gpu.py drives), 1.5 mm and 0.03 degrees of
    drift per node, uniform odometry weights and a loop edge that carries the true relative pose with weight 1e6: the optimum
    is the truth, keyframe errors fall below 1 % of the drifted ones (measured: 4e-8 of them).

    Two things bound what any optimiser can do here, and both are asserted as what they are.  With the loop edge weighted like
    an odometry edge it takes its 1 / 24 share of the discrepancy, and 1 / 24 of the error stays.  And with the cameras ON a
    circle of 1 m the residual is a twist in each camera's own frame, so that the quadratic cost mixes rotation and translation
    through the lever arm between the nodes: spreading the discrepancy evenly over the edges is then no longer the linear
    drift's inverse, and the optimum - the gradient test below shows it is one - keeps 12 % of the translation error."""
    truth, drifted, edges = linear_drift_case(0.0, 1e6)
    out, rep = pg.optimize(drifted, edges)
    (before, rot_before), (after, rot_after) = errors(drifted, truth), errors(out, truth)
    print(f"ring: translation error max {before.max():.5f} -> {after.max():.3e} m, rotation max {rot_before:.6f} -> {rot_after:.3e} rad; "
          f"{rep['iterations']} iterations")
    assert rep["cost_after"] < rep["cost_before"]
    assert np.sqrt((after ** 2).mean()) < 0.01 * np.sqrt((before ** 2).mean())
    assert after.max() < 0.01 * before.max() and rot_after < 0.01 * rot_before
    assert len(rep["residual_norms_before"]) == len(edges) == len(rep["residual_norms_after"])
    assert rep["residual_norms_before"][-1] > 10 * max(rep["residual_norms_before"][:-1])          # the loop edge held all of it
    # the loop edge weighted like the others keeps its share
    truth, drifted, edges = linear_drift_case(0.0, 1.0)
    out, _ = pg.optimize(drifted, edges)
    after1, rot1 = errors(out, truth)
    assert abs(after1.max() / before.max() - 1 / RING) < 1e-3 and abs(rot1 / rot_before - 1 / RING) < 1e-3
    # on a circle of 1 m the optimum improves the poses without restoring them
    truth, drifted, edges = linear_drift_case(1.0, 1e6)
    out, _ = pg.optimize(drifted, edges, iterations=40)
    (b, rb), (a, ra) = errors(drifted, truth), errors(out, truth)
    print(f"ring of 1 m: translation error max {b.max():.5f} -> {a.max():.5f} m, rotation max {rb:.5f} -> {ra:.5f} rad")
    assert a.max() < 0.25 * b.max() and ra < rb


def test_gradient_vanishes_at_the_result():
    truth, drifted, edges = ring_case(w_rot=3.0, w_trans=0.7)
    out, _ = pg.optimize(drifted, edges, iterations=40)
    h = 1e-5
    worst = 0.0
    for n in range(1, RING):
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            plus, minus = out.copy(), out.copy()
            plus[n] = out[n] @ se3_exp(d)
            minus[n] = out[n] @ se3_exp(-d)
            worst = max(worst, abs(pg.cost(plus, edges) - pg.cost(minus, edges)) / (2 * h))
    print("largest gradient entry at the optimum:", worst)
    assert worst < 1e-8


@pytest.mark.parametrize("fixed", [0, 7])
def test_fixed_node_does_not_move(fixed):
    truth, drifted, edges = ring_case()
    out, _ = pg.optimize(drifted, edges, fixed=fixed)
    assert np.array_equal(out[fixed], drifted[fixed])
    assert np.abs(out[(fixed + 5) % RING] - drifted[(fixed + 5) % RING]).max() > 1e-4


def test_huber_limits_a_wrong_loop_edge():
    truth = ring_truth()
    edges = [(k - 1, k, pg.inverse(truth[k - 1]) @ truth[k], 1.0, 1.0) for k in range(1, RING)]
    wrong = pg.inverse(truth[-1]) @ truth[0] @ se3_exp([0.0, 0.2, 0.0, 0.5, 0.0, 0.0])
    edges.append((RING - 1, 0, wrong, 1.0, 1.0, True))
    plain, _ = pg.optimize(truth, edges, iterations=40)
    robust, rep = pg.optimize(truth, edges, iterations=40, huber=0.01)
    moved_plain, moved_robust = trans_err(plain, truth).max(), trans_err(robust, truth).max()
    print(f"wrong loop edge: largest move {moved_plain:.4f} m without Huber, {moved_robust:.4f} m with")
    assert moved_robust < moved_plain                 # a pull of 2 huber on a chain of 23 unit springs: about 23 huber
    assert moved_robust < 2 * 23 * 0.01
    assert rep["cost_after"] <= rep["cost_before"]
    unmarked = [e[:5] for e in edges]
    same, _ = pg.optimize(truth, unmarked, iterations=40, huber=0.01)               # the mark decides, not the option alone
    assert np.abs(same - plain).max() < 1e-9


def test_bad_arguments():
    truth = ring_truth()
    Z = np.eye(4)
    for edges, kw in (([(0, 0, Z, 1.0, 1.0)], {}), ([(0, RING, Z, 1.0, 1.0)], {}), ([(0, 1, Z, -1.0, 1.0)], {}),
                      ([(0, 1, Z, 1.0, 1.0)], {"fixed": RING}), ([(0, 1, Z, 1.0, 1.0)], {"huber": 0.0})):
        with pytest.raises(ValueError):
            pg.optimize(truth, edges, **kw)
