"""Generates tests/golden/history_merge_ref.npz: the REFERENCE's own Mapping.history_merge (mapper.py:212-251, imported
through oracle/ref_shim.py) run on CPU on the seeded inputs of `inputs()`, with a stand-in `self` carrying exactly the
attributes the method reads.  Build container only; the outputs are committed so
tests/test_oracle_slam_ops.py::test_history_merge_oracle_equals_the_reference_method runs anywhere.

    python oracle/gen_history_merge_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "history_merge_ref.npz")
WEIGHT = 0.5


def inputs(N=500):
    """Packed map rows then / now, with rotations on both sides of the slerp's colinearity threshold, and confidences."""
    gen = torch.Generator().manual_seed(4)
    then = dict(xyz=torch.randn(N, 3, generator=gen), shs=torch.randn(N, 48, generator=gen), raw8=torch.randn(N, 8, generator=gen))
    now = {k: v + 0.05 * torch.randn(v.shape, generator=gen) for k, v in then.items()}
    now["raw8"][:50, 4:8] = then["raw8"][:50, 4:8] * 1.3          # colinear rotations: the lerp branch
    now["raw8"][50:100, 4:8] = torch.randn(50, 4, generator=gen)  # far apart: the slerp branch
    c_then = torch.randint(0, 40, (N, 1), generator=gen).float()
    c_now = c_then + torch.randint(0, 51, (N, 1), generator=gen).float()
    return then, now, c_then, c_now


def reference_outputs():
    from types import SimpleNamespace
    from oracle import ref_shim
    mp = ref_shim.load("SLAM.multiprocess.mapper")
    F = torch.nn.functional
    then, now, c_then, c_now = inputs()
    N = then["xyz"].shape[0]
    pc = SimpleNamespace(get_confidence=c_now, get_xyz=now["xyz"], _features_dc=now["shs"].view(N, 16, 3)[:, :1].clone(),
                         _features_rest=now["shs"].view(N, 16, 3)[:, 1:].clone(), _scaling=now["raw8"][:, 1:4].clone(),
                         get_rotation=F.normalize(now["raw8"][:, 4:8]))
    me = SimpleNamespace(pointcloud=pc, verbose=False)
    hist = dict(confidence=c_then, xyz=then["xyz"], features_dc=then["shs"].view(N, 16, 3)[:, :1],
                features_rest=then["shs"].view(N, 16, 3)[:, 1:], scaling=then["raw8"][:, 1:4],
                rotation=F.normalize(then["raw8"][:, 4:8]))
    mp.Mapping.history_merge(me, hist, WEIGHT)
    return {"xyz": pc._xyz.numpy(), "shs": torch.cat([pc._features_dc, pc._features_rest], 1).reshape(N, 48).numpy(),
            "scaling": pc._scaling.numpy(), "rotation": pc._rotation.numpy()}


def main():
    np.savez_compressed(PATH, **reference_outputs())


if __name__ == "__main__":
    main()
