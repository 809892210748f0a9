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
    bench_ab   as above.

--keypoints measures the keypoint registration (rtg_slam_amd/keypoints.py, csrc/keypoints.hip) instead -> profiles/r28_keypoints.json:

    kernels    rtgs_keypoint_detect + rtgs_keypoint_describe per keyframe at 320x240, 600x340 and 1200x680 of the textured room
               (the two launches alone, and keypoints.detect_and_describe with its copy of the slots to the host), and
               rtgs_keypoint_match for 1 and 64 candidate pairs (both directions each: 2 and 128 query sets) at about 300 and
               about 3 000 keypoints a side: device events, a warm-up, 5 blocks; median and range per launch.
    sequence   the tour above in the TEXTURED room (synth.box_room_texture_color), loop_closure_candidates appearance, once with
               loop_closure_appearance_init yaw and once with keypoints: candidates, accepted edges, each edge's distance from
               the stream's true relative pose, where every first guess came from, ATE RMSE plain and aligned before and after.
    bench_ab   as above.

--sh measures the rotation of the SH bands (rtg_slam_amd/sh_rotation.py, csrc/map_deform_sh.hip) instead
-> profiles/r31_sh_rotation.json:

    kernels    rtgs_map_deform_sh at 300 000 and 1 200 000 rows over a 2 000-frame table with every row flagged, int32 ticks
               in ascending runs (a real map: the waves share one frame) and drawn at random (the worst case: every lane gathers
               its own matrix): device events, a warm-up, 5 blocks of CALLS launches; median and range per launch and the
               counted bytes per second (360 B a moved row: 45 floats in and out).  Beside it, in the same process and with the
               same ticks, rtgs_map_deform (60 B a row) and the plain torch form the kernel replaces - the [N,7,7], [N,5,5] and
               [N,3,3] matrices gathered by tick and three batched products.  And the host time of sh_rotation_table for the
               2 000 frames.
    bench_ab   as above.

--texture runs the sequence of any arm in the textured room."""
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


def time_sh_kernels(dev):
    import time
    import numpy as np
    import torch
    from rtg_slam_amd import _lib, loop_closure as lc, sh_rotation as shr
    from rtg_slam_amd.rgbd_align import se3_exp
    lib = _lib.load()
    step = se3_exp([0.0, np.deg2rad(1.0) / TABLE_FRAMES, 0.0, 0.05 / TABLE_FRAMES, 0.0, 0.0])
    D, cur = [], np.eye(4)
    for _ in range(TABLE_FRAMES):                                             # the drift of time_kernels: to 1 degree and 5 cm
        cur = cur @ step
        D.append(cur.copy())
    D = np.stack(D)
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        sh_np = shr.sh_rotation_table(D)
        host.append(time.perf_counter() - t0)
    assert sh_np[:, 83].all()
    sh_table = torch.from_numpy(sh_np).to(dev)
    table = torch.from_numpy(lc.deform_table(D)).to(dev)
    M = [sh_table[:, at:at + n * n].reshape(-1, n, n).contiguous() for n, at in ((3, 0), (5, 9), (7, 34))]

    def blocks(call):
        for _ in range(20):
            call()
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
        return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    out = {"sh_rotation_table_host_ms": {"frames": TABLE_FRAMES, "median": round(1e3 * statistics.median(host), 2),
                                         "min": round(1e3 * min(host), 2), "max": round(1e3 * max(host), 2)}, "rows": [],
           "what": "launch-to-launch times of back-to-back launches on the same rows: 58 MB of SH rows at 300 k and 230 MB at 1.2 M "
                   "stay in or near the 256 MiB Infinity Cache between launches, so the counted TB/s are not HBM rates"}
    for N in (300_000, 1_200_000):
        g = torch.Generator(device="cpu").manual_seed(1)
        shs = (torch.randn(N, 16, 3, generator=g) * 0.05).to(dev)
        xyz = (torch.rand(N, 3, generator=g) * 4 - 2).to(dev)
        raw8 = torch.randn(N, 8, generator=g).to(dev)
        ticks = {"runs": ((torch.arange(N, dtype=torch.int64) * TABLE_FRAMES) // N).to(torch.int32),
                 "random": torch.randint(0, TABLE_FRAMES, (N,), generator=g, dtype=torch.int32)}
        for name, tick in ticks.items():
            tick = tick.to(dev)
            long_tick = tick.long()

            def kernel():
                assert lib.rtgs_map_deform_sh(_lib.ptr(shs), _lib.ptr(tick), 0, N, _lib.ptr(sh_table), TABLE_FRAMES, _lib.stream(dev)) == 0

            def rigid():
                assert lib.rtgs_map_deform(_lib.ptr(xyz), _lib.ptr(raw8), _lib.ptr(tick), 0, N, _lib.ptr(table), TABLE_FRAMES,
                                           _lib.stream(dev)) == 0

            def torch_form():
                for (first, n), m in zip(((1, 3), (4, 5), (9, 7)), M):
                    shs[:, first:first + n] = torch.bmm(m[long_tick], shs[:, first:first + n])
            row = {"rows": N, "ticks": name, "table_frames": TABLE_FRAMES, "calls_per_block": CALLS, "blocks": BLOCKS,
                   "us_per_launch": {"rtgs_map_deform_sh": blocks(kernel), "rtgs_map_deform": blocks(rigid), "torch_form": blocks(torch_form)},
                   "note": "per launch = host enqueue included; every row is moved; the rows are turned in place again and again by "
                           "orthogonal matrices, so they keep their size"}
            us = row["us_per_launch"]
            row["counted_TB_per_s_at_median"] = {"rtgs_map_deform_sh (360 B a row)": round(360 * N / us["rtgs_map_deform_sh"]["median"] * 1e-6, 3),
                                                 "rtgs_map_deform (60 B a row)": round(60 * N / us["rtgs_map_deform"]["median"] * 1e-6, 3),
                                                 "torch_form (360 B a row)": round(360 * N / us["torch_form"]["median"] * 1e-6, 3)}
            row["kernel_beats_torch_form"] = bool(us["rtgs_map_deform_sh"]["median"] < us["torch_form"]["median"])
            row["finite"] = bool(torch.isfinite(shs).all())
            out["rows"].append(row)
            print(row, flush=True)
    return out


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


def time_keypoint_kernels(dev):
    import numpy as np
    import torch
    from rtg_slam_amd import _lib, keypoints as kp, synth
    lib = _lib.load()

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

    out = {"detect_describe": [], "match": []}
    cfg = kp.config()
    dirs, tables = kp._device_tables(dev)
    pose = synth.trajectory(2, seed=21)[0]
    for H, W in ((240, 320), (340, 600), (680, 1200)):
        s = W / synth.REPLICA.W
        cam = synth.CameraSpec(H, W, synth.REPLICA.fx * s, synth.REPLICA.fy * s, (W - 1) / 2.0, (H - 1) / 2.0)
        d = synth.box_room_depth(cam, pose, device=dev)
        c = synth.box_room_texture_color(cam, pose, d).contiguous()
        d = d.reshape(1, H, W).contiguous()
        K = np.array([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1.0]])
        f = kp.detect_and_describe(c, d, K, cfg, keep_planes=True)
        n_slots = int(f["slots"].shape[0])
        g8, box, slots, desc = f["g8"], f["box5"], f["slots"], f["slot_desc"]

        def launches():
            lib.rtgs_keypoint_detect(_lib.ptr(c), _lib.ptr(d), H, W, cfg.cell, cfg.threshold, _lib.ptr(g8), _lib.ptr(box), _lib.ptr(slots),
                                     _lib.stream(dev))
            lib.rtgs_keypoint_describe(_lib.ptr(g8), _lib.ptr(box), H, W, n_slots, 1, _lib.ptr(dirs), _lib.ptr(tables), _lib.ptr(slots),
                                       _lib.ptr(desc), _lib.stream(dev))
        row = {"H": H, "W": W, "cell": cfg.cell, "slots": n_slots, "keypoints": int(len(f["x"])), "calls_per_block": CALLS, "blocks": BLOCKS,
               "us_per_keyframe_two_launches": blocks(launches, CALLS),
               "us_per_keyframe_detect_and_describe": blocks(lambda: kp.detect_and_describe(c, d, K, cfg), CALLS),
               "bytes": 21 * H * W, "note": "two launches = host enqueue included; detect_and_describe adds the compaction on the "
                                            "device and the copy of the keypoints to the host, which waits for the device"}
        row["GB_per_s_two_launches_at_median"] = round(row["bytes"] / row["us_per_keyframe_two_launches"]["median"] * 1e-3, 1)
        out["detect_describe"].append(row)
        print(row, flush=True)
    for n, pairs, calls in ((300, 1, CALLS), (300, 64, CALLS), (3000, 1, CALLS), (3000, 64, 10)):
        g = torch.Generator(device="cpu").manual_seed(n + pairs)
        all_desc = torch.randint(-2 ** 31, 2 ** 31 - 1, (2 * pairs * n, 8), generator=g, dtype=torch.int64).to(torch.int32).to(dev)
        table = []
        for k in range(pairs):                                                    # sets 2 k and 2 k + 1, both directions
            table.append((2 * k * n, n, (2 * k + 1) * n, n, 2 * k * n))
            table.append(((2 * k + 1) * n, n, 2 * k * n, n, (2 * k + 1) * n))
        tab = torch.tensor(table, dtype=torch.int32).to(dev)
        res = torch.empty((2 * pairs * n, 3), dtype=torch.int32, device=dev)
        call = lambda: lib.rtgs_keypoint_match(_lib.ptr(all_desc), 2 * pairs * n, _lib.ptr(tab), 2 * pairs, n, _lib.ptr(res), 2 * pairs * n,
                                               _lib.stream(dev))
        assert call() == 0
        row = {"keypoints_a_side": n, "candidate_pairs": pairs, "query_sets": 2 * pairs, "distances": 2 * pairs * n * n,
               "calls_per_block": calls, "blocks": BLOCKS, "us_per_launch": blocks(call, calls)}
        row["distances_per_s_at_median"] = round(row["distances"] / row["us_per_launch"]["median"] * 1e6)
        out["match"].append(row)
        print(row, flush=True)
    return out


def sequence(dev, frames, mode=None, texture=False, init=None, levels=None):
    import numpy as np
    import torch
    from rtg_slam_amd import mapping as mp, slam, synth
    cam = synth.REPLICA
    poses = synth.room_tour(frames, seed=21)

    def stream(n):
        for c2w in poses[:n]:
            d = synth.box_room_depth(cam, c2w, device=dev)
            c = synth.box_room_texture_color(cam, c2w, d) if texture else synth.box_room_color(cam, c2w, d)
            torch.cuda.synchronize(dev)
            yield d.reshape(cam.H, cam.W), c, c2w.numpy()

    slam.run_sequence(cam, stream(30), mp.replica_args(seed=1), dev, capacity=800_000)         # warm-up, thrown away
    args = mp.replica_args(seed=1, loop_closure=True, **({} if mode is None else {"loop_closure_candidates": mode}),
                           **({} if init is None else {"loop_closure_appearance_init": init}),
                           **({} if levels is None else {"loop_closure_keypoint_levels": levels}))
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
        if "keypoint_search" in lcr:                              # candidates keypoints: pairs voted, shortlisted, seconds per stage
            out["keypoint_search"] = lcr["keypoint_search"]
        ids = [int(i) for i in mapper.keyframe_ids]
        for row, c in zip(out["candidate_list"], lcr["candidates"]):
            row.update({k: c[k] for k in ("source", "score", "shift", "depth_rel", "init_source", "keypoints", "votes") if k in c})
            want = pg.inverse(np.asarray(tracker.pose_gt[ids[c["a"]]], dtype=np.float64)) @ np.asarray(tracker.pose_gt[ids[c["b"]]])
            row["true_angle_deg"] = float(np.rad2deg(np.arccos(min(1.0, max(-1.0, (np.trace(want[:3, :3]) - 1.0) / 2.0)))))
            row["true_distance_m"] = float(np.linalg.norm(want[:3, 3]))
            row["z_error_m"] = float(np.linalg.norm(np.asarray(c["Z"])[:3, 3] - want[:3, 3])) if c.get("Z") is not None else None
            if "init" in c:
                row["init_error_m"] = float(np.linalg.norm(np.asarray(c["init"])[:3, 3] - want[:3, 3]))
        out["by_source"] = {s: {"candidates": sum(r.get("source", "pose") == s for r in out["candidate_list"]),
                                "accepted": sum(r.get("source", "pose") == s and r["accepted"] for r in out["candidate_list"])}
                            for s in ("pose", "appearance", "keypoints")}
        out["wrong_edges"] = [(r["a"], r["b"]) for r in out["candidate_list"] if r["accepted"] and r["z_error_m"] is not None and r["z_error_m"] > 0.05]
    if "graph" in lcr:
        g = lcr["graph"]
        out["graph"] = {k: g[k] for k in ("cost_before", "cost_after", "iterations", "accepted", "last_update", "reason")}
    out["run"] = {"ate_rmse_m": rep["ate_rmse_m"], "ate_rmse_aligned_m": rep["ate_rmse_aligned_m"], "gaussians": rep["gaussians"],
                  "fps": rep["fps"], "wall_s": rep["wall_s"]}
    out["what"] = (f"slam.run_sequence, {frames} frames of synth.room_tour(seed=21) in the box room at {cam.W}x{cam.H}, "
                   "replica_args(seed=1, loop_closure=True) from an empty map, ICP tracking, every loop_closure_* value at its default"
                   + ("" if mode is None else f" but loop_closure_candidates = {mode}")
                   + ("" if init is None else f" and loop_closure_appearance_init = {init}")
                   + ("" if levels is None else f" and loop_closure_keypoint_levels = {levels}")
                   + (", in the textured room (synth.box_room_texture_color)" if texture else ""))
    print({k: v for k, v in out.items() if k != "candidate_list"}, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--appearance", action="store_true", help="measure the place recognition instead (r27_place_recognition.json)")
    ap.add_argument("--keypoints", action="store_true", help="measure the keypoint registration instead (r28_keypoints.json)")
    ap.add_argument("--keypoint-search", action="store_true",
                    help="run the textured sequence with loop_closure_candidates keypoints at --levels levels (r30_keypoint_pyramid_tour.json)")
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--sh", action="store_true", help="measure the rotation of the SH bands instead (r31_sh_rotation.json)")
    ap.add_argument("--texture", action="store_true", help="run the sequence in the textured room (always so with --keypoints)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="kernels,sequence", help="what to measure now; an existing --out file keeps its other parts")
    opts = ap.parse_args()
    parts = set(opts.parts.split(","))
    opts.out = opts.out or os.path.join(ROOT, "profiles", "r31_sh_rotation.json" if opts.sh else "r30_keypoint_pyramid_tour.json" if opts.keypoint_search else "r28_keypoints.json" if opts.keypoints else
                                        "r27_place_recognition.json" if opts.appearance else "r26_loop_closure.json")
    result = json.load(open(opts.out)) if os.path.exists(opts.out) else {}
    if opts.parent_tree:                                      # first: this process has not opened the GPU yet
        result["bench_ab"] = rac.bench_ab(os.path.abspath(opts.parent_tree), opts.ab_runs)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loop_closure_check.py needs a GPU; nothing was measured")
    dev = torch.device("cuda", 0)
    result["device"] = torch.cuda.get_device_name(dev)
    if opts.sh:                                               # no sequence of its own: the tour's closure is r26's
        if "kernels" in parts:
            result["kernels"] = time_sh_kernels(dev)
        parts = set()
    if opts.keypoint_search:                                  # its kernels are timed by tools/keypoint_pyramid_check.py
        result["sequence"] = sequence(dev, opts.frames, "keypoints", True, levels=opts.levels)
        parts = set()
    if "kernels" in parts:
        result["kernels"] = (time_keypoint_kernels(dev) if opts.keypoints else time_place_kernels(dev) if opts.appearance
                             else time_kernels(dev))
    if "sequence" in parts and opts.keypoints:
        result["sequence"] = {init: sequence(dev, opts.frames, "appearance", True, init) for init in ("yaw", "keypoints")}
    elif "sequence" in parts and opts.appearance:
        result["sequence"] = {mode: sequence(dev, opts.frames, mode, opts.texture) for mode in ("pose", "appearance", "both")}
    elif "sequence" in parts:
        result["sequence"] = sequence(dev, opts.frames, texture=opts.texture)
    with open(opts.out, "w") as f:
        json.dump(result, f, indent=1, default=float)
        f.write("\n")
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
