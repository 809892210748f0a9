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

    python tools/loop_closure_check.py [--frames 2000] [--parent-tree DIR] [--ab-runs 3] [--parts kernels,sequence] [--out FILE]

--appearance measures the place recognition (rtg_slam_amd/place_recognition.py, csrc/place.hip) instead
-> profiles/r27_place_recognition.json:

    kernels    rtgs_place_describe at 320x240, 600x340 and 1200x680 (thumbnail width 40) and rtgs_place_scores at 71, 500 and
               2 000 random descriptors of 40 x 23 cells (min_gap 10, 4 shifts to either side): device events, a warm-up, 5
               blocks; median and range per launch, and pairs per second.
    sequence   the tour above once per loop_closure_candidates mode (pose, appearance, both; loop_closure_huber off): candidates
               by source, accepted edges, how far every measured appearance edge lies from the stream's true relative pose,
               ATE RMSE plain and aligned before and after, seconds per stage.
    bench_ab   as above."""
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


def time_place_kernels(dev):
    import torch
    from rtg_slam_amd import place_recognition as pr, synth

    def blocks(call, calls):
        for _ in range(3):
            call()
        torch.cuda.synchronize(dev)
        us = []
        for _ in range(BLOCKS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                call()
            b.record()
            b.synchronize()
            us.append(1e3 * a.elapsed_time(b) / calls)
        return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    out = {"describe": [], "scores": []}
    pose = synth.trajectory(2, seed=21)[0]
    for H, W in ((240, 320), (340, 600), (680, 1200)):
        s = W / synth.REPLICA.W
        cam = synth.CameraSpec(H, W, synth.REPLICA.fx * s, synth.REPLICA.fy * s, (W - 1) / 2.0, (H - 1) / 2.0)
        d = synth.box_room_depth(cam, pose, device=dev)
        c = synth.box_room_color(cam, pose, d).contiguous()
        d = d.reshape(1, H, W).contiguous()
        desc = pr.describe(c, d, 40)
        row = {"H": H, "W": W, "thumbnail": [40, int(desc["intensity"].shape[1])], "calls_per_block": CALLS, "blocks": BLOCKS,
               "us_per_launch": blocks(lambda: pr.describe(c, d, 40, out=desc), CALLS), "bytes_read": 16 * H * W,
               "note": "per launch = host enqueue and the Python wrapper included; one keyframe per launch"}
        row["GB_per_s_at_median"] = round(row["bytes_read"] / row["us_per_launch"]["median"] * 1e-3, 1)
        out["describe"].append(row)
        print(row, flush=True)
    for M, calls in ((71, CALLS), (500, 10), (2000, 3)):
        g = torch.Generator(device="cpu").manual_seed(M)
        desc = {k: torch.rand(M, 23, 40, generator=g).to(dev) for k in ("intensity", "depth", "valid")}
        mats = pr.score_pairs(desc, 10, 4)
        pairs = sum(max(0, b - 9) for b in range(M))
        row = {"keyframes": M, "cells": [40, 23], "max_shift": 4, "min_gap": 10, "pairs": pairs, "calls_per_block": calls,
               "blocks": BLOCKS, "us_per_launch": blocks(lambda: pr.score_pairs(desc, 10, 4, out=mats), calls)}
        row["pairs_per_s_at_median"] = round(pairs / row["us_per_launch"]["median"] * 1e6)
        row["pair_shifts_per_s_at_median"] = 9 * row["pairs_per_s_at_median"]
        out["scores"].append(row)
        print(row, flush=True)
    return out


def sequence(dev, frames, mode=None):
    import numpy as np
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
    args = mp.replica_args(seed=1, loop_closure=True, **({} if mode is None else {"loop_closure_candidates": mode}))
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
    if mode is not None:
        from rtg_slam_amd import pose_graph as pg
        out["mode"], out["appearance"] = mode, lcr.get("appearance")
        ids = [int(i) for i in mapper.keyframe_ids]
        for row, c in zip(out["candidate_list"], lcr["candidates"]):
            row.update({k: c[k] for k in ("source", "score", "shift", "depth_rel") if k in c})
            want = pg.inverse(np.asarray(tracker.pose_gt[ids[c["a"]]], dtype=np.float64)) @ np.asarray(tracker.pose_gt[ids[c["b"]]])
            row["true_angle_deg"] = float(np.rad2deg(np.arccos(min(1.0, max(-1.0, (np.trace(want[:3, :3]) - 1.0) / 2.0)))))
            row["true_distance_m"] = float(np.linalg.norm(want[:3, 3]))
            row["z_error_m"] = float(np.linalg.norm(np.asarray(c["Z"])[:3, 3] - want[:3, 3])) if "Z" in c else None
        out["by_source"] = {s: {"candidates": sum(r.get("source", "pose") == s for r in out["candidate_list"]),
                                "accepted": sum(r.get("source", "pose") == s and r["accepted"] for r in out["candidate_list"])}
                            for s in ("pose", "appearance")}
    if "graph" in lcr:
        g = lcr["graph"]
        out["graph"] = {k: g[k] for k in ("cost_before", "cost_after", "iterations", "accepted", "last_update", "reason")}
    out["run"] = {"ate_rmse_m": rep["ate_rmse_m"], "ate_rmse_aligned_m": rep["ate_rmse_aligned_m"], "gaussians": rep["gaussians"],
                  "fps": rep["fps"], "wall_s": rep["wall_s"]}
    out["what"] = (f"slam.run_sequence, {frames} frames of synth.room_tour(seed=21) in the box room at {cam.W}x{cam.H}, "
                   "replica_args(seed=1, loop_closure=True) from an empty map, ICP tracking, every loop_closure_* value at its default"
                   + ("" if mode is None else f" but loop_closure_candidates = {mode}"))
    print({k: v for k, v in out.items() if k != "candidate_list"}, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--appearance", action="store_true", help="measure the place recognition instead (r27_place_recognition.json)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="kernels,sequence", help="what to measure now; an existing --out file keeps its other parts")
    opts = ap.parse_args()
    parts = set(opts.parts.split(","))
    opts.out = opts.out or os.path.join(ROOT, "profiles", "r27_place_recognition.json" if opts.appearance else "r26_loop_closure.json")
    result = json.load(open(opts.out)) if os.path.exists(opts.out) else {}
    if opts.parent_tree:                                      # first: this process has not opened the GPU yet
        result["bench_ab"] = rac.bench_ab(os.path.abspath(opts.parent_tree), opts.ab_runs)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loop_closure_check.py needs a GPU; nothing was measured")
    dev = torch.device("cuda", 0)
    result["device"] = torch.cuda.get_device_name(dev)
    if "kernels" in parts:
        result["kernels"] = time_place_kernels(dev) if opts.appearance else time_kernels(dev)
    if "sequence" in parts and opts.appearance:
        result["sequence"] = {mode: sequence(dev, opts.frames, mode) for mode in ("pose", "appearance", "both")}
    elif "sequence" in parts:
        result["sequence"] = sequence(dev, opts.frames)
    with open(opts.out, "w") as f:
        json.dump(result, f, indent=1, default=float)
        f.write("\n")
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
