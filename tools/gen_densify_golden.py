"""Regenerate tests/golden/densify_ref.npz: the reference's own GaussianPointCloud.densify (SLAM/gaussian_pointcloud.py:53-116)
run on the CPU over 48 stable Gaussians, for (sigma, circle_num, levels) in (1, 30, 5), (2, 7, 3), (3, 1, 1).

Build container only (needs the reference tree; oracle/ref_mapper_shim.py imports its modules in place, unchanged).  Open3D
is stubbed by a PointCloud that keeps the arrays it is given.  The torch seed is fixed before each call and theta is
recorded by drawing it again from the same seed, as densify draws it (torch.rand(1, C) * pi * 2).

The rows: random, equal in-plane scales (two equal larger scales, as every new Gaussian starts: xyz_factor [1, 1, 0.1]),
all three scales equal, and a tie at the minimum.

    python tools/gen_densify_golden.py          # writes tests/golden/densify_ref.npz
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = ((1, 30, 5), (2, 7, 3), (3, 1, 1))
SEED = 1234


class _PointCloud:
    def __init__(self):
        self.points = None
        self.normals = None


def _rows(n_each: int = 12, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(4 * n_each, 3, generator=g) * 2.0
    rot = torch.randn(4 * n_each, 4, generator=g)
    raw = torch.randn(n_each, 3, generator=g) * 0.7 - 3.0                   # random
    eq = torch.randn(n_each, 1, generator=g) * 0.5 - 3.0                     # equal in-plane scales, a smaller third one
    in_plane = torch.cat([eq, eq, eq + np.log(0.1)], dim=1)
    perm = [torch.randperm(3, generator=g) for _ in range(n_each)]
    in_plane = torch.stack([in_plane[i, perm[i]] for i in range(n_each)])
    all_eq = (torch.randn(n_each, 1, generator=g) * 0.5 - 3.0).repeat(1, 3)  # all three equal
    lo = torch.randn(n_each, 1, generator=g) * 0.5 - 4.0                     # a tie at the minimum
    hi = lo + 0.5 + torch.rand(n_each, 1, generator=g)
    min_tie = torch.cat([lo, lo, hi], dim=1)
    min_tie = torch.stack([min_tie[i, torch.randperm(3, generator=g)] for i in range(n_each)])
    scaling = torch.cat([raw, in_plane, all_eq, min_tie]).float()
    return xyz.float(), scaling, rot.float()


def main(out_path: str = os.path.join(ROOT, "tests", "golden", "densify_ref.npz")) -> None:
    from oracle import ref_mapper_shim
    ref_mapper_shim.install()
    o3d = sys.modules["open3d"]
    o3d.geometry = types.SimpleNamespace(PointCloud=_PointCloud)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.array(a))
    gp = sys.modules["SLAM.gaussian_pointcloud"]
    xyz, scaling, rot = _rows()
    pc = object.__new__(gp.GaussianPointCloud)
    pc.setup_functions()
    pc._xyz, pc._scaling, pc._rotation = xyz, scaling, rot
    out = {"xyz": xyz.numpy(), "scaling": scaling.numpy(), "rotation": rot.numpy(),
           "scales": pc.get_scaling.numpy(), "rotations": pc.get_rotation.numpy(), "cases": np.array(CASES, np.int32)}
    for i, (sigma, C, L) in enumerate(CASES):
        torch.manual_seed(SEED + i)
        theta = torch.rand(1, C) * torch.pi * 2
        torch.manual_seed(SEED + i)
        pcd = pc.densify(sigma, C, L)
        out[f"theta_{i}"] = theta[0].numpy()
        out[f"cos_{i}"] = torch.cos(theta)[0].numpy()
        out[f"sin_{i}"] = torch.sin(theta)[0].numpy()
        out[f"points_{i}"] = np.asarray(pcd.points, dtype=np.float32)
        out[f"normals_{i}"] = np.asarray(pcd.normals, dtype=np.float32)
        assert out[f"points_{i}"].shape == (xyz.shape[0] * sigma * C * L, 3)
    np.savez_compressed(out_path, **out)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
