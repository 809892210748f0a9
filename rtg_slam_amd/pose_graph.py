"""Pose-graph optimisation on the host (numpy float64): the back end `loop_closure.LoopCloser` hands its keyframe poses and its
odometry and loop edges to.

    nodes     c2w 4x4 matrices T_0 .. T_{M-1}
    edge      (a, b, Z, w_rot, w_trans[, robust]): T_a^-1 T_b should be Z
    residual  r = se3_log(Z^-1 T_a^-1 T_b), a twist (rotation first, as rgbd_align.se3_exp / se3_log)
    cost      sum over the edges of rho(e^2), e^2 = w_rot |r_rot|^2 + w_trans |r_trans|^2; rho is the identity, or - on the edges
              marked robust, when `huber` is given - Huber's function of the weighted residual norm e: e^2 up to e = huber,
              2 huber e - huber^2 beyond

Levenberg-Marquardt on the manifold: node i moves as T_i exp(d_i), the normal equations are dense (6 M unknowns, M a few
hundred), the node `fixed` is held.  The Jacobian of the residual is exact: log(E exp(d)) = r + J_r^-1(r) d with J_r(r) =
sum_n (-ad_r)^n / (n + 1)!, summed as a series of the 6 x 6 matrix ad_r.  Robust edges are re-weighted at every linearisation
(iteratively re-weighted least squares).  No scipy."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .rgbd_align import se3_exp, se3_log


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def inverse(T) -> np.ndarray:
    """Inverse of a rigid 4x4 transform."""
    T = np.asarray(T, dtype=np.float64)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def adjoint(T) -> np.ndarray:
    """Ad(T) for twists (w, v): T exp(x) T^-1 = exp(Ad(T) x)."""
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = _hat(t) @ R
    return A


def right_jacobian_inverse(r) -> np.ndarray:
    """J_r^-1(r): se3_log(exp(r) exp(d)) = r + J_r^-1(r) d to first order."""
    ad = np.zeros((6, 6))
    ad[:3, :3] = ad[3:, 3:] = _hat(r[:3])
    ad[3:, :3] = _hat(r[3:])
    J, term = np.eye(6), np.eye(6)
    for n in range(1, 60):
        term = term @ (-ad) / (n + 1.0)
        J = J + term
        if np.abs(term).max() < 1e-18:
            break
    return np.linalg.inv(J)


def _parse(edges):
    out = []
    for e in edges:
        a, b, Z, w_rot, w_trans = e[:5]
        robust = bool(e[5]) if len(e) > 5 else False
        if int(a) == int(b):
            raise ValueError("pose_graph: an edge joins two different nodes")
        if not (w_rot >= 0 and w_trans >= 0):
            raise ValueError("pose_graph: edge weights must not be negative")
        out.append((int(a), int(b), np.asarray(Z, dtype=np.float64).reshape(4, 4), float(w_rot), float(w_trans), robust))
    return out


def residuals(poses, edges) -> np.ndarray:
    """[E, 6]: r of every edge at `poses`."""
    poses = np.asarray(poses, dtype=np.float64)
    return np.array([se3_log(inverse(Z) @ inverse(poses[a]) @ poses[b]) for a, b, Z, _, _, _ in _parse(edges)]).reshape(-1, 6)


def _edge_costs(r, parsed, huber):
    """-> (rho(e^2) per edge, the IRLS factor per edge)."""
    w = np.array([[e[3]] * 3 + [e[4]] * 3 for e in parsed]).reshape(-1, 6)
    e2 = (w * r * r).sum(1)
    rho, fac = e2.copy(), np.ones(len(parsed))
    if huber is not None:
        k = float(huber)
        for i, e in enumerate(parsed):
            if e[5] and e2[i] > k * k:
                en = np.sqrt(e2[i])
                rho[i] = 2.0 * k * en - k * k
                fac[i] = k / en
    return rho, fac


def cost(poses, edges, huber: Optional[float] = None) -> float:
    parsed = _parse(edges)
    return float(_edge_costs(residuals(poses, parsed), parsed, huber)[0].sum()) if parsed else 0.0


def optimize(poses, edges: Sequence, fixed: int = 0, iterations: int = 20, tol: float = 1e-10,
             huber: Optional[float] = None) -> Tuple[np.ndarray, Dict]:
    """-> (poses_new [M,4,4] float64, report).  The loop ends after `iterations` accepted or refused steps, when the largest
    entry of an accepted update is at most `tol`, or when the damping can grow no further.  report: "cost_before" /
    "cost_after", "iterations" (linearisations), "accepted", "last_update" (the largest entry of the last accepted update; 0
    when none was needed), "residual_norms_before" / "_after" (|r| per edge, unweighted), "reason"."""
    T = np.array(poses, dtype=np.float64).reshape(-1, 4, 4)
    M = T.shape[0]
    parsed = _parse(edges)
    if not 0 <= int(fixed) < M:
        raise ValueError("pose_graph: the fixed node is not a node")
    for a, b, *_ in parsed:
        if not (0 <= a < M and 0 <= b < M):
            raise ValueError("pose_graph: an edge names a node that does not exist")
    if huber is not None and not huber > 0:
        raise ValueError("pose_graph: huber must be positive (None = off)")
    free = [i for i in range(M) if i != int(fixed)]
    col = {n: 6 * k for k, n in enumerate(free)}

    def evaluate(Tc):
        r = np.array([se3_log(inverse(Z) @ inverse(Tc[a]) @ Tc[b]) for a, b, Z, _, _, _ in parsed]).reshape(-1, 6)
        rho, fac = _edge_costs(r, parsed, huber)
        return r, float(rho.sum()), fac

    r, c, fac = evaluate(T)
    rep = {"cost_before": c, "residual_norms_before": [float(np.sqrt(np.dot(x, x))) for x in r], "iterations": 0, "accepted": 0,
           "last_update": 0.0, "reason": "iterations"}
    lam = 1e-6
    for _ in range(int(iterations)):
        if not parsed or not free:
            rep["reason"] = "nothing to optimise"
            break
        rep["iterations"] += 1
        H, g = np.zeros((6 * len(free), 6 * len(free))), np.zeros(6 * len(free))
        for i, (a, b, Z, w_rot, w_trans, _) in enumerate(parsed):
            W = np.array([w_rot] * 3 + [w_trans] * 3) * fac[i]
            Jb = right_jacobian_inverse(r[i])
            Ja = -Jb @ adjoint(inverse(T[b]) @ T[a])
            for n, Jn in ((a, Ja), (b, Jb)):
                if n not in col:
                    continue
                g[col[n]:col[n] + 6] += Jn.T @ (W * r[i])
                for m, Jm in ((a, Ja), (b, Jb)):
                    if m in col:
                        H[col[n]:col[n] + 6, col[m]:col[m] + 6] += Jn.T @ (W[:, None] * Jm)
        if np.abs(g).max() <= 1e-15:
            rep["reason"] = "converged"
            break
        stepped = False
        while lam < 1e12:
            try:
                d = np.linalg.solve(H + lam * np.diag(np.diag(H)) + 1e-12 * lam * np.eye(len(g)), -g)
            except np.linalg.LinAlgError:
                lam *= 10.0
                continue
            Tn = T.copy()
            for n in free:
                Tn[n] = T[n] @ se3_exp(d[col[n]:col[n] + 6])
            rn, cn, facn = evaluate(Tn)
            if np.isfinite(cn) and cn <= c:
                T, r, c, fac = Tn, rn, cn, facn
                lam = max(lam / 10.0, 1e-12)
                rep["accepted"] += 1
                rep["last_update"] = float(np.abs(d).max())
                stepped = True
                break
            lam *= 10.0
        if not stepped:
            rep["reason"] = "no step lowers the cost"
            break
        if rep["last_update"] <= tol:
            rep["reason"] = "converged"
            break
    rep["cost_after"] = c
    rep["residual_norms_after"] = [float(np.sqrt(np.dot(x, x))) for x in r]
    return T, rep
