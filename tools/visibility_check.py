"""Times the visibility cull (evaluation.VisibilityCull) on the device and prints one JSON line (also written to OUT when given):
  * .add per frame at 1200 x 680 (the Replica camera in the box room, poses of synth.room_tour, the room's own depth) on the
    flat room's wall grid (tests/visibility_reference.box_grid) at about 1 M and about 5 M vertices; the vertices a frame sees
    are counted from the counts' change, the bytes moved are 12 B per vertex (its position) plus 4 B gathered per projected
    vertex and 8 B per seen vertex (its count, read and written);
  * .mesh() (the keep flags, torch's scans, the compaction kernels and the host's reads of the two counts) with the counts
    before and after.
Timing: device events around `reps` calls, after a warm-up of 3, in `blocks` blocks; the median block and the spread of the
blocks are reported.  python tools/visibility_check.py [OUT] [reps = 10] [blocks = 5]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtg_slam_amd import evaluation, synth   # noqa: E402
from tests import visibility_reference as vr   # noqa: E402


def blocks_ms(fn, reps, blocks, warmup=3):
    """fn(i) launches the i-th call; -> per-call milliseconds of every block."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(reps):
            fn(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return {"median_ms": round(float(np.median(out)), 4), "min_ms": round(float(np.min(out)), 4),
            "max_ms": round(float(np.max(out)), 4), "reps_per_block": reps, "blocks": blocks}


def main():
    argv = sys.argv[1:]
    out_path = argv[0] if len(argv) > 0 else None
    reps = int(argv[1]) if len(argv) > 1 else 10
    blocks = int(argv[2]) if len(argv) > 2 else 5
    dev = torch.device("cuda", 0)
    cam = synth.REPLICA
    res = {"device": torch.cuda.get_device_name(dev), "camera": [cam.W, cam.H], "tolerance": 0.1,
           "timing": "device events around reps .add calls (the host's 4x4 inverse and the launch included), blocks after a "
                     "warm-up of 3 calls; .mesh() is wall clock with a final synchronise"}
    poses = synth.room_tour(reps * 40, seed=3)[::40]
    frames = [(synth.box_room_depth(cam, p, device=dev).reshape(cam.H, cam.W).contiguous(), p.numpy()) for p in poses]
    for name, cell in (("room_1M", 0.0112), ("room_5M", 0.00502)):
        v, f = vr.box_grid(vr.ROOM_HALF, cell=cell)
        V = len(v)
        cull = evaluation.VisibilityCull(v, f, cam, tolerance=0.1, device=dev)
        del v, f
        seen, projected = [], []
        for d, p in frames:
            before = cull.views.clone()
            cull.add(d, p)
            seen.append(int((cull.views != before).sum()))
        # what projects into the image at all: everything does against an infinitely far surface, nothing against holes
        probe = evaluation.VisibilityCull(cull.vertices, cull.faces[:0], cam, tolerance=0.1, device=dev)
        far, total = torch.full_like(frames[0][0], float("inf")), 0
        for d, p in frames:
            probe.add(far, p)
            probe.add(torch.zeros_like(far), p)
            projected.append(int(probe.views.sum()) - total)
            total += projected[-1]
        del probe, far
        entry = {"cell": cell, "V": V, "F": int(cull.faces.shape[0]), "seen_per_frame_mean": int(np.mean(seen)),
                 "projected_per_frame_mean": int(np.mean(projected))}
        moved = 12.0 * V + 4.0 * float(np.mean(projected)) + 8.0 * float(np.mean(seen))
        entry["bytes_moved_per_frame_mean"] = int(moved)
        t = blocks_ms(lambda i: cull.add(*frames[i % len(frames)]), reps, blocks)
        t["GB_per_s_of_moved_bytes_at_median"] = round(moved / (t["median_ms"] * 1e-3) / 1e9, 1)
        entry["add"] = t
        ms = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cv, cf = cull.mesh()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        entry["mesh"] = {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                         "runs": 3, "V_kept": int(cv.shape[0]), "F_kept": int(cf.shape[0])}
        entry["report"] = cull.report()
        res[name] = entry
        del cull, cv, cf
        torch.cuda.empty_cache()
    line = json.dumps(res, default=float)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            json.dump(res, fo, indent=1, default=float)


if __name__ == "__main__":
    main()
