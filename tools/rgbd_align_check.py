"""What the RGB-D refinement (rtg_slam_amd/rgbd_align.py) costs and what it changes, on one MI355X -> profiles/r22_rgbd_align.json.

    accumulate   rtgs_rgbd_align_accumulate (both launches) beside rtgs_icp_step on the same maps at 300x170, 600x340 and
                 1200x680: blocks of CALLS calls between two device events, the two kinds of block alternating, the median block
                 and the range of the blocks per call.
    sequence     slam.run_sequence over FRAMES frames of the box-room tour at 1200x680 (bench.py's sequence leg) without and
                 with rgbd_refine: tracking_s_mean, ATE, the refinement's host reads, iterations and ms per frame.
    bench_ab     with --parent-tree DIR (a checkout of the parent commit with its library built): `bench.py --gpus 1 --steps 20
                 --warmup 3` in fresh processes, parent and this tree alternating; the default path is untouched, so the median
                 of this tree should lie inside the parent's range.

    python tools/rgbd_align_check.py [--frames 300] [--parent-tree DIR] [--out profiles/r22_rgbd_align.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((170, 300), (340, 600), (680, 1200))
CALLS, BLOCKS = 200, 7


def bench_ab(parent, runs):
    rows = []
    for i in range(runs):
        for arm, tree in (("parent", parent), ("this", ROOT)):
            env = dict(os.environ, PYTHONPATH=tree)
            r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"],
                               cwd=tree, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"bench.py failed in {tree}: {r.stderr[-2000:]}")
            line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            rows.append({"run": i, "arm": arm, "ms_per_step": line["ms_per_step"], "value": line["value"]})
            print(rows[-1], flush=True)
    out = {"command": "bench.py --gpus 1 --steps 20 --warmup 3, fresh processes, parent and this tree alternating", "runs": rows}
    for arm in ("parent", "this"):
        ms = sorted(r["ms_per_step"] for r in rows if r["arm"] == arm)
        out[arm] = {"median_ms_per_step": statistics.median(ms), "min": ms[0], "max": ms[-1]}
    out["this_median_inside_parent_range"] = out["parent"]["min"] <= out["this"]["median_ms_per_step"] <= out["parent"]["max"]
    return out


def time_accumulate(dev):
    import numpy as np
    import torch
    from rtg_slam_amd import icp, rgbd_align, synth
    rows = []
    poses = synth.trajectory(2, seed=9)
    base = synth.look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3)
    cos = float(np.cos(np.deg2rad(20.0)))
    for H, W in SIZES:
        s = W / synth.REPLICA.W
        cam = synth.CameraSpec(H, W, synth.REPLICA.fx * s, synth.REPLICA.fy * s, (W - 1) / 2.0, (H - 1) / 2.0)
        K = torch.tensor([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=torch.float32, device=dev)
        maps = []
        for p in (base @ poses[1], base @ poses[0]):                                  # source t1, target t0
            d = synth.box_room_depth(cam, p, device=dev)
            v, n = icp.build_pyramids(d, K, 1)
            maps += [v[0], n[0], rgbd_align.intensity_pyramid(synth.box_room_color(cam, p, d), 1)[0]]
        vs, ns, i_s, vt, nt, i_t = maps
        pose = torch.eye(4, device=dev)
        lib = rgbd_align._lib.load()
        scratch = torch.empty(lib.rtgs_rgbd_align_scratch_bytes(H, W) // 8, dtype=torch.float64, device=dev)

        def joint():
            return rgbd_align.accumulate(vs, ns, i_s, vt, nt, i_t, K, pose, 0.1, cos, 0.25, 0.05, scratch)

        def step():
            return icp.icp_step(vs, ns, vt, nt, K, pose, 0.1, cos)

        sums = joint().cpu().numpy()
        _, _, nv = step()
        for f in (joint, step):                                                       # warm both shapes
            for _ in range(20):
                f()
        torch.cuda.synchronize(dev)
        us = {"joint": [], "icp_step": []}
        for _ in range(BLOCKS):
            for name, f in (("joint", joint), ("icp_step", step)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(CALLS):
                    f()
                b.record()
                b.synchronize()
                us[name].append(1e3 * a.elapsed_time(b) / CALLS)
        row = {"H": H, "W": W, "calls_per_block": CALLS, "blocks": BLOCKS, "geometric_inliers": int(sums[28]),
               "photometric_inliers": int(sums[30]), "icp_step_valid": int(nv.item())}
        for name, v in us.items():
            row[name + "_us_per_call"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        row["note"] = ("per call = host enqueue included (the blocks are launch-bound at the small sizes): joint = 2 launches + the "
                       "allocation of its 31-double result, icp_step = its launches + three result tensors")
        rows.append(row)
        print(row, flush=True)
    return rows


def sequence(dev, frames):
    import torch
    from rtg_slam_amd import mapping as mp, slam, synth
    cam = synth.REPLICA
    poses = synth.room_tour(frames, seed=21)
    out = {}
    # the first arm is a short run that is thrown away: it pays for the code objects and the allocator's first blocks
    for name, over, n in (("warm_up", {"rgbd_refine": True}, 30), ("icp_only", {}, frames), ("rgbd_refine", {"rgbd_refine": True}, frames)):
        args = mp.replica_args(seed=1, **over)

        def stream():
            for c2w in poses[:n]:
                d = synth.box_room_depth(cam, c2w, device=dev)
                c = synth.box_room_color(cam, c2w, d)
                torch.cuda.synchronize(dev)
                yield d.reshape(cam.H, cam.W), c, c2w.numpy()

        _, tracker, rep = slam.run_sequence(cam, stream(), args, dev, capacity=800_000)
        del tracker
        if name == "warm_up":
            continue
        row = {k: rep[k] for k in ("frames", "tracking_s_mean", "mapping_s_mean", "fps", "ate_rmse_m", "ate_rmse_aligned_m",
                                   "final_translation_error_m")}
        row["tracker_host_reads_per_frame"] = 1 + (rep["rgbd_refine"]["host_reads_mean"] if "rgbd_refine" in rep else 0)
        if "rgbd_refine" in rep:
            row["rgbd_refine"] = rep["rgbd_refine"]
        out[name] = row
        print(name, row, flush=True)
    out["what"] = (f"slam.run_sequence, {frames} frames of synth.room_tour(seed=21) in the box room at {cam.W}x{cam.H}, clean depth, "
                   "replica_args(seed=1), from an empty map; tracker_host_reads_per_frame = ICP's one read + the refinement's")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_rgbd_align.json"))
    opts = ap.parse_args()
    result = {}
    if opts.parent_tree:                                      # first: this process has not opened the GPU yet
        result["bench_ab"] = bench_ab(os.path.abspath(opts.parent_tree), opts.ab_runs)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rgbd_align_check.py needs a GPU; nothing was measured")
    dev = torch.device("cuda", 0)
    result["device"] = torch.cuda.get_device_name(dev)
    result["accumulate"] = time_accumulate(dev)
    result["sequence"] = sequence(dev, opts.frames)
    with open(opts.out, "w") as f:
        json.dump(result, f, indent=1, default=float)
        f.write("\n")
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
