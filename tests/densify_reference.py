"""A torch (CPU, float32) restatement of the stable cloud's densification (SLAM/gaussian_pointcloud.py:53-116 with get_normal /
get_plane :539-571), step for step in the order include/rtgs_slam.h ("densification") gives, to check the rtgs_densify_discs
kernel against.  Pinned itself to the reference's own output by tests/golden/densify_ref.npz (tools/gen_densify_golden.py)."""
from __future__ import annotations

import torch


def frames(scales: torch.Tensor, rotations: torch.Tensor):
    """-> n, p0, p1 [P,3] (unit columns of R for the smallest, middle and largest scale; ties to the lower axis index) and
    a0, a1 [P] (the middle and the largest scale)."""
    s = scales.float()
    q = rotations.float()
    qn = torch.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    r, x, y, z = (q[:, i] / qn for i in range(4))
    R = torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], dim=1),
        torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], dim=1),
        torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1)], dim=1)
    order = torch.sort(s, dim=1, stable=True).indices
    cols = R.transpose(1, 2)                                   # cols[:, j] = column j of R
    ar = torch.arange(s.shape[0])

    def unit(j):
        v = cols[ar, order[:, j]]
        return v / (torch.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) + 1e-8)[:, None]

    return unit(0), unit(1), unit(2), s[ar, order[:, 1]], s[ar, order[:, 2]]


def densify(xyz, scales, rotations, cos, sin, sigma: int, levels: int):
    """-> points, normals float32 [P K, 3], K = sigma levels C, Gaussian-major, point k = s (L C) + l C + c."""
    xyz = xyz.float()
    cos, sin = cos.float().reshape(-1), sin.float().reshape(-1)
    C, L = int(cos.numel()), int(levels)
    K = int(sigma) * L * C
    n, p0, p1, a0, a1 = frames(scales, rotations)
    k = torch.arange(K)
    c, l, ring = k % C, (k // C) % L, k // (L * C)
    lf = torch.tensor([(i + 0.5) / L for i in range(L)], dtype=torch.float64).float()[l]
    a = (a0 * sigma)[:, None] * lf[None] + a0[:, None] * ring.float()[None]
    b = (a1 * sigma)[:, None] * lf[None] + a1[:, None] * ring.float()[None]
    px, pz = a * cos[c][None], b * sin[c][None]
    off = [(v[:, 0, None] * px + v[:, 1, None] * 0.0) + v[:, 2, None] * pz for v in (p0, n, p1)]
    pts = torch.stack(off, dim=-1) + xyz[:, None, :]
    return pts.reshape(-1, 3), n[:, None, :].expand(-1, K, 3).reshape(-1, 3)


def close(got, want, rel: float = 1e-6) -> float:
    """Largest |got - want| / max(1, |want|) over the rows (the |.| of a row is its largest component)."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    scale = want.abs().amax(dim=-1, keepdim=True).clamp_min(1.0)
    return float(((got - want).abs() / scale).max()) if want.numel() else 0.0
