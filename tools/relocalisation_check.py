"""Measurements of the device RANSAC and the relocaliser on the GPU -> profiles/r29_relocalisation.json.

    python tools/relocalisation_check.py [--parts kernels,locate,tour] [--frames 2000] [--parent-tree DIR] [--ab-runs 3] [--out FILE]

    kernels    rtgs_rigid_ransac for 1, 3 and 64 pairs at 60, 120 and 1000 matches, 512 hypotheses: device events, a warm-up, 5
               blocks, median and range per launch; beside it keypoints.ransac_rigid (the host's RANSAC) on the same matches
    locate     one whole Relocaliser.locate call against 71 and 500 keyframes of the textured box-room tour at 1200 x 680, split by
               stage: the first call (the candidates' keypoints are computed) and the median of 5 more (they are kept)
    tour       slam.run_sequence over FRAMES frames of the textured tour (synth.room_tour(seed=21), replica_args(seed=1)), once
               undisturbed without the option, once with relocalise and 10 covered frames (depth and colour zero) INSERTED after
               each quarter of the tour - the camera stands still while covered: frames lost, frames to recovery, the events, and
               the ATE over the tracked frames beside the undisturbed run's; and once more with icp_fail_threshold infinite, so
               that only the covered frames are lost
    bench_ab   with --parent-tree: bench.py --gpus 1 --steps 20 --warmup 3 in fresh processes, the parent's tree and this one
               alternating (the option is off there)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rgbd_align_check as rac                                                # noqa: E402  (bench_ab)

BLOCKS, COVERED = 5, 10


def synthetic_pairs(pairs, n, seed):
    """`pairs` pairs of n mutual matches each (none filtered out): a rigid motion, 5 mm of noise, two in five gross outliers."""
    import numpy as np
    from rtg_slam_amd.rgbd_align import se3_exp
    rng = np.random.default_rng(seed)
    T = se3_exp([0.1, -0.3, 0.05, 0.4, -0.2, 0.3])
    tabs, pts, table = [], [], []
    for p in range(pairs):
        xb = rng.uniform(-2, 2, size=(n, 3)) + (0, 0, 3)
        xa = xb @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.005, (n, 3))
        bad = rng.permutation(n)[:(2 * n) // 5]
        xa[bad] += rng.uniform(0.5, 2.0, size=(len(bad), 3)) * rng.choice([-1, 1], size=(len(bad), 3))
        m = np.stack([np.arange(n), np.full(n, 20), np.full(n, 100)], axis=1).astype(np.int32)
        table.append((2 * p * n, n, (2 * p + 1) * n, n, 2 * p * n, (2 * p + 1) * n))
        tabs += [m, m]
        pts += [xa, xb]
    return np.concatenate(tabs), np.concatenate(pts), table


def time_kernels(dev):
    import numpy as np
    import torch
    from rtg_slam_amd import _lib, keypoints as kp
    lib = _lib.load()
    rows = []
    for n in (60, 120, 1000):
        host_ms = None
        for pairs in (1, 3, 64):
            m, x, table = synthetic_pairs(pairs, n, n + pairs)
            matches, xyz = torch.from_numpy(m).to(dev), torch.from_numpy(x).to(dev)
            tab = torch.tensor(table, dtype=torch.int32).to(dev)
            cap = min(n + (n & 1), kp.RANSAC_CAP)
            out = torch.empty((pairs, kp.RANSAC_HEAD + 3 * cap), dtype=torch.int32, device=dev)
            call = lambda: lib.rtgs_rigid_ransac(_lib.ptr(matches), int(matches.shape[0]), _lib.ptr(xyz), int(xyz.shape[0]), _lib.ptr(tab), pairs,
                                                 64, 0.8, 512, 0.05, 0, cap, _lib.ptr(out), _lib.stream(dev))
            calls = 20 if n < 1000 else 10
            for _ in range(3):
                assert call() == 0
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
            fits = kp.rigid_ransac_tables(matches, xyz, table, dev)
            if host_ms is None:                                                # the host's RANSAC on the first pair's matches
                xa, xb = x[table[0][4]:table[0][4] + n], x[table[0][5]:table[0][5] + n]
                ms = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    fit = kp.ransac_rigid(xa, xb, 512, 0.05)
                    ms.append(1e3 * (time.perf_counter() - t0))
                host_ms = {"median": round(statistics.median(ms), 2), "min": round(min(ms), 2), "max": round(max(ms), 2),
                           "inliers": int(fit[1].sum()), "device_inliers": fits[0]["inliers"],
                           "max_abs_T_difference": float(np.abs(fit[0] - fits[0]["T"]).max())}
            med = statistics.median(us)
            row = {"pairs": pairs, "matches": n, "hypotheses": 512, "calls_per_block": calls, "blocks": BLOCKS,
                   "us_per_launch": {"median": round(med, 2), "min": round(min(us), 2), "max": round(max(us), 2)},
                   "us_per_pair_at_median": round(med / pairs, 2), "host_ransac_rigid_ms_per_pair": host_ms,
                   "host_over_device_per_pair": round(1e3 * host_ms["median"] / (med / pairs), 1),
                   "note": "per launch = host enqueue included; the host's figure is one pair, 3 runs"}
            rows.append(row)
            print(row, flush=True)
    return rows


def time_locate(dev, search=None, levels=None):
    import numpy as np
    import torch
    from types import SimpleNamespace
    from rtg_slam_amd import mapping as mp, relocalisation as rl, synth
    from rtg_slam_amd.rgbd_align import se3_exp
    cam = synth.REPLICA
    rows = []
    for M in (71, 500):
        poses = synth.room_tour(M, seed=21)
        keymaps = []
        for c2w in poses:
            d = synth.box_room_depth(cam, c2w, device=dev)
            keymaps.append({"color_chw": synth.box_room_texture_color(cam, c2w, d).contiguous(), "depth_chw": d.reshape(1, cam.H, cam.W).contiguous()})
        mapper = SimpleNamespace(keymap_list=keymaps, keyframe_list=[mp.Frame(cam, poses[0].numpy(), dev)], keyframe_ids=list(range(M)))
        tracker = SimpleNamespace(pose_es=[p.numpy().astype(np.float64) for p in poses])
        r = rl.Relocaliser(mp.replica_args(seed=1, relocalise=True, **({} if search is None else {"relocalise_search": search}),
                                            **({} if levels is None else {"relocalise_keypoint_levels": levels})))
        r.mapper = mapper
        r.on_keyframes(mapper)
        a = M // 2
        truth = poses[a].numpy().astype(np.float64) @ se3_exp([0.0, np.deg2rad(3.0), 0.0, 0.04, -0.02, 0.03])
        d = synth.box_room_depth(cam, torch.from_numpy(truth), device=dev)
        fm = {"color_chw": synth.box_room_texture_color(cam, torch.from_numpy(truth), d).contiguous(), "depth_chw": d.reshape(1, cam.H, cam.W).contiguous()}
        torch.cuda.synchronize(dev)
        calls = []
        for k in range(6):
            before = dict(r.seconds)
            t0 = time.perf_counter()
            pose = r.locate(tracker, fm, M + k)
            torch.cuda.synchronize(dev)
            total = time.perf_counter() - t0
            calls.append(dict({s: 1e3 * (r.seconds[s] - before[s]) for s in r.seconds}, total=1e3 * total))
        ev = r.events[-1] if r.events else None
        row = {"keyframes": M, "image": [cam.W, cam.H], "recovered": pose is not None, "refusals": dict(r.refusals),
               "error_mm": None if pose is None else 1e3 * float(np.linalg.norm(pose[:3, 3] - truth[:3, 3])),
               "event": None if ev is None else {k: ev[k] for k in ("keyframe", "score", "votes", "matches", "inliers", "correction_trans") if k in ev},
               "first_call_ms": {k: round(v, 3) for k, v in calls[0].items()},
               "later_calls_ms_median": {k: round(statistics.median(c[k] for c in calls[1:]), 3) for k in calls[0]},
               "later_calls_ms_max": {k: round(max(c[k] for c in calls[1:]), 3) for k in calls[0]},
               "note": "every stage ends with a device synchronisation; later calls find the candidates' keypoints kept"}
        rows.append(row)
        print(row, flush=True)
        del keymaps, mapper, r
        torch.cuda.empty_cache()
    return rows


def tour(dev, frames):
    import numpy as np
    import torch
    from rtg_slam_amd import mapping as mp, slam, synth
    cam = synth.REPLICA
    poses = synth.room_tour(frames, seed=21)
    gaps = [frames // 4, frames // 2, (3 * frames) // 4]

    def stream(n, covered):
        for k, c2w in enumerate(poses[:n]):
            if covered and k in gaps:
                for _ in range(COVERED):
                    yield (torch.zeros((cam.H, cam.W), device=dev), torch.zeros((3, cam.H, cam.W), device=dev), poses[k - 1].numpy())
            d = synth.box_room_depth(cam, c2w, device=dev)
            c = synth.box_room_texture_color(cam, c2w, d)
            torch.cuda.synchronize(dev)
            yield d.reshape(cam.H, cam.W), c, c2w.numpy()

    slam.run_sequence(cam, stream(30, False), mp.replica_args(seed=1), dev, capacity=800_000)         # warm-up, thrown away
    out = {}
    # the third arm: only singular equations and a non-finite pose lose a frame - icp_fail_threshold (0.02 in replica_args)
    # flags frames of this tour that the undisturbed run tracks through
    for name, covered, over in (("undisturbed", False, {}), ("covered", True, {"relocalise": True}),
                                ("covered_fail_threshold_off", True, {"relocalise": True, "icp_fail_threshold": float("inf")})):
        _, tracker, rep = slam.run_sequence(cam, stream(frames, covered), mp.replica_args(seed=1, **over), dev, capacity=800_000)
        row = {"frames": rep["frames"], "keyframes": rep["keyframes"], "ate_rmse_m": rep["ate_rmse_m"], "fps": rep["fps"],
               "tracking_ms_mean": 1e3 * rep["tracking_s_mean"], "mapping_ms_mean": 1e3 * rep["mapping_s_mean"], "gaussians": rep["gaussians"]}
        if covered:
            rl_ = rep["relocalisation"]
            row.update(ate_rmse_tracked_m=rep["ate_rmse_tracked_m"], lost_frames=len(rl_["lost_frames"]), attempts=rl_["attempts"],
                       refusals=rl_["refusals"], seconds=rl_["seconds"], covered_after_frames=gaps, covered_frames_each=COVERED,
                       events=[dict({k: e[k] for k in e if k != "Z"}, frames_lost=e["recovered_at"] - e["lost_at"]) for e in rl_["events"]],
                       still_lost_at_the_end=bool(tracker.lost))
        out[name] = row
        print(name, row, flush=True)
    out["what"] = (f"slam.run_sequence, {frames} frames of synth.room_tour(seed=21) in the textured box room at {cam.W}x{cam.H}, replica_args(seed=1) "
                   f"from an empty map, ICP tracking; covered: relocalise on, {COVERED} frames of zero depth and colour inserted before frames {gaps}")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_relocalisation.json"))
    ap.add_argument("--search", choices=("thumbnails", "keypoints"), default=None, help="relocalise_search of the locate part")
    ap.add_argument("--levels", type=int, default=None, help="relocalise_keypoint_levels of the locate part")
    ap.add_argument("--parts", default="kernels,locate,tour", help="what to measure now; an existing --out file keeps its other parts")
    opts = ap.parse_args()
    parts = set(opts.parts.split(","))
    result = json.load(open(opts.out)) if os.path.exists(opts.out) else {}
    if opts.parent_tree:                                      # first: this process has not opened the GPU yet
        result["bench_ab"] = rac.bench_ab(os.path.abspath(opts.parent_tree), opts.ab_runs)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("relocalisation_check.py needs a GPU; nothing was measured")
    dev = torch.device("cuda", 0)
    result["device"] = torch.cuda.get_device_name(dev)
    if "kernels" in parts:
        result["kernels"] = time_kernels(dev)
    if "locate" in parts:
        key = "locate" if opts.search is None and opts.levels is None else f"locate_{opts.search or 'thumbnails'}_levels_{opts.levels or 1}"
        result[key] = time_locate(dev, opts.search, opts.levels)
    if "tour" in parts:
        result["tour"] = tour(dev, opts.frames)
    with open(opts.out, "w") as f:
        json.dump(result, f, indent=1, default=float)
        f.write("\n")
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
