"""What the loop closure (rtg_slam_amd/loop_closure.py, csrc/map_deform.hip) costs and what it changes, on one MI355X
-> profiles/r26_loop_closure.json.

    kernels    rtgs_map_deform alone at 300 000 and 1 200 000 rows, int32 ticks spread over 2 000 frames in runs (the rows a
               frame added sit together), every row moved: device events, a warm-up, then 5 blocks of CALLS launches; median and
               range in microseconds per launch and the counted bytes per second (60 B a row: xyz and rotation in and out, the
               tick; the 64-B table rows come from the cache).
    sequence   slam.run_sequence with loop_closure on over FRAMES frames of the box-room tour of BASELINE.json configs[2]
               (bench.py's sequence leg: synth.room_tour(seed=21), 1200x680, replica_args(seed=1), empty map): keyframes,
               candidates, accepted edges and the refusals by reason, the graph report, seconds per stage, ATE RMSE plain and
               aligned before and after.
    bench_ab   with --parent-tree DIR (a built checkout of the parent commit): bench.py in alternating fresh processes.

    python tools/loop_closure_check.py [--frames 2000] [--parent-tree DIR] [--ab-runs 3] [--parts kernels,sequence] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rgbd_align_check as rac                                                # noqa: E402  (bench_ab)

CALLS, BLOCKS, TABLE_FRAMES = 50, 5, 2000


def time_kernels(dev):
    import numpy as np
    import torch
    from rtg_slam_amd import _lib, loop_closure as lc
    from rtg_slam_amd.rgbd_align import se3_exp
    lib = _lib.load()
    rows = []
    step = se3_exp([0.0, np.deg2rad(1.0) / TABLE_FRAMES, 0.0, 0.05 / TABLE_FRAMES, 0.0, 0.0])
    D, cur = [], np.eye(4)
    for _ in range(TABLE_FRAMES):                                             # a drift that grows to 1 degree and 5 cm
        cur = cur @ step
        D.append(cur.copy())
    table = torch.from_numpy(lc.deform_table(np.stack(D))).to(dev)
    for N in (300_000, 1_200_000):
        g = torch.Generator(device="cpu").manual_seed(1)
        xyz = (torch.rand(N, 3, generator=g) * 4 - 2).to(dev)
        raw8 = torch.randn(N, 8, generator=g).to(dev)
        tick = ((torch.arange(N, dtype=torch.int64) * TABLE_FRAMES) // N).to(torch.int32).to(dev)
        call = lambda: lib.rtgs_map_deform(_lib.ptr(xyz), _lib.ptr(raw8), _lib.ptr(tick), 0, N, _lib.ptr(table), TABLE_FRAMES,
                                           _lib.stream(dev))
        for _ in range(20):
            assert call() == 0
        torch.cuda.synchronize(dev)
        us = []
        for _ in range(BLOCKS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                call()
            b.record()
            b.synchronize()
            us.append(1e3 * a.elapsed_time(b) / CALLS)
        med = statistics.median(us)
        row = {"rows": N, "table_frames": TABLE_FRAMES, "calls_per_block": CALLS, "blocks": BLOCKS,
               "us_per_launch": {"median": round(med, 2), "min": round(min(us), 2), "max": round(max(us), 2)},
               "counted_bytes_per_row": 60, "counted_GB_per_s_at_median": round(60 * N / med * 1e-3, 1),
               "finite": bool(torch.isfinite(xyz).all() and torch.isfinite(raw8).all()),
               "note": "per launch = host enqueue included; every row is moved (no identity row in the table)"}
        rows.append(row)
        print(row, flush=True)
    return rows


def sequence(dev, frames):
    import torch
    from rtg_slam_amd import mapping as mp, slam, synth
    cam = synth.REPLICA
    poses = synth.room_tour(frames, seed=21)

    def stream(n):
        for c2w in poses[:n]:
            d = synth.box_room_depth(cam, c2w, device=dev)
            c = synth.box_room_color(cam, c2w, d)
            torch.cuda.synchronize(dev)
            yield d.reshape(cam.H, cam.W), c, c2w.numpy()

    slam.run_sequence(cam, stream(30), mp.replica_args(seed=1), dev, capacity=800_000)         # warm-up, thrown away
    args = mp.replica_args(seed=1, loop_closure=True)
    mapper, tracker, rep = slam.run_sequence(cam, stream(frames), args, dev, capacity=800_000)
    lcr = rep["loop_closure"]
    reasons = {}
    for c in lcr["candidates"]:
        key = c["reason"].split(" ")[0] if c["accepted"] else " ".join(c["reason"].split(" ")[:2])
        reasons[key] = reasons.get(key, 0) + 1
    out = {k: lcr.get(k) for k in ("frames", "keyframes", "edges", "changed", "options", "exposure_unknowns", "seconds",
                                   "correction_max_m", "correction_mean_m", "correction_max_deg", "ate_rmse_m_before", "ate_rmse_m",
                                   "ate_rmse_aligned_m_before", "ate_rmse_aligned_m")}
    out["candidates"] = len(lcr["candidates"])
    out["outcomes"] = reasons
    out["candidate_list"] = [{k: c[k] for k in ("a", "b", "frame_a", "frame_b", "distance_m", "angle_deg", "accepted", "reason",
                                                "inlier_ratio", "rms_geometric_after", "correction_trans", "correction_rot_deg")}
                             for c in lcr["candidates"]]
    if "graph" in lcr:
        g = lcr["graph"]
        out["graph"] = {k: g[k] for k in ("cost_before", "cost_after", "iterations", "accepted", "last_update", "reason")}
    out["run"] = {"ate_rmse_m": rep["ate_rmse_m"], "ate_rmse_aligned_m": rep["ate_rmse_aligned_m"], "gaussians": rep["gaussians"],
                  "fps": rep["fps"], "wall_s": rep["wall_s"]}
    out["what"] = (f"slam.run_sequence, {frames} frames of synth.room_tour(seed=21) in the box room at {cam.W}x{cam.H}, "
                   "replica_args(seed=1, loop_closure=True) from an empty map, ICP tracking, every loop_closure_* value at its default")
    print({k: v for k, v in out.items() if k != "candidate_list"}, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_loop_closure.json"))
    ap.add_argument("--parts", default="kernels,sequence", help="what to measure now; an existing --out file keeps its other parts")
    opts = ap.parse_args()
    parts = set(opts.parts.split(","))
    result = json.load(open(opts.out)) if os.path.exists(opts.out) else {}
    if opts.parent_tree:                                      # first: this process has not opened the GPU yet
        result["bench_ab"] = rac.bench_ab(os.path.abspath(opts.parent_tree), opts.ab_runs)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loop_closure_check.py needs a GPU; nothing was measured")
    dev = torch.device("cuda", 0)
    result["device"] = torch.cuda.get_device_name(dev)
    if "kernels" in parts:
        result["kernels"] = time_kernels(dev)
    if "sequence" in parts:
        result["sequence"] = sequence(dev, opts.frames)
    with open(opts.out, "w") as f:
        json.dump(result, f, indent=1, default=float)
        f.write("\n")
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
