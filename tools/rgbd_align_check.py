"""What the RGB-D refinement (rtg_slam_amd/rgbd_align.py) costs and what it changes, on one MI355X -> profiles/r22_rgbd_align.json.

    accumulate   rtgs_rgbd_align_accumulate (both launches) beside rtgs_icp_step on the same maps at 300x170, 600x340 and
                 1200x680: blocks of CALLS calls between two device events, the two kinds of block alternating, the median block
                 and the range of the blocks per call.
    sequence     slam.run_sequence over FRAMES frames of the box-room tour at 1200x680 (bench.py's sequence leg) without and
                 with rgbd_refine: tracking_s_mean, ATE, the refinement's host reads, iterations and ms per frame.
    bench_ab     with --parent-tree DIR (a checkout of the parent commit with its library built): `bench.py --gpus 1 --steps 20
                 --warmup 3` in fresh processes, parent and this tree alternating; the default path is untouched, so the median
                 of this tree should lie inside the parent's range.

    python tools/rgbd_align_check.py [--frames 300] [--parent-tree DIR] [--out profiles/r22_rgbd_align.json]

With --exposure it measures the exposure compensation and the model-colour target instead -> profiles/r23_rgbd_exposure.json:

    accumulate   rtgs_rgbd_align_accumulate_exposure (48 sums) beside rtgs_rgbd_align_accumulate (31) on the same maps, and
                 rtgs_rgbd_target_intensity beside rtgs_rgbd_intensity_pyramid (three levels), in alternating blocks:
                 EXPOSURE_BLOCKS blocks after a warm-up, the median block and the range.
    sequence     the four arms - plain, exposure, model, both - over FRAMES frames of the same tour: tracker ms per frame,
                 evaluations per frame, ATE; once on the clean colour and once with a per-frame gain / offset walk on it.
    bench_ab     as above.

    python tools/rgbd_align_check.py --exposure [--frames 300] [--parent-tree DIR]"""
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
EXPOSURE_BLOCKS = 5
ARMS = (("plain", {}), ("exposure", {"rgbd_refine_exposure": True}), ("model", {"rgbd_refine_target": "model"}),
        ("both", {"rgbd_refine_exposure": True, "rgbd_refine_target": "model"}))


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


def _alternating(fns, blocks, calls):
    """{name: f} -> {name: {"median", "min", "max"}} in microseconds per call: warm-up, then `blocks` rounds in which every f
    runs `calls` times between two device events."""
    import torch
    for f in fns.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in fns}
    for _ in range(blocks):
        for name, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            us[name].append(1e3 * a.elapsed_time(b) / calls)
    return {name: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for name, v in us.items()}


def time_exposure(dev):
    import numpy as np
    import torch
    from rtg_slam_amd import icp, rgbd_align, synth
    rows = []
    poses = synth.trajectory(2, seed=9)
    base = synth.look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3)
    cos = float(np.cos(np.deg2rad(20.0)))
    lib = rgbd_align._lib.load()
    for H, W in SIZES:
        s = W / synth.REPLICA.W
        cam = synth.CameraSpec(H, W, synth.REPLICA.fx * s, synth.REPLICA.fy * s, (W - 1) / 2.0, (H - 1) / 2.0)
        K = torch.tensor([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=torch.float32, device=dev)
        maps, colours, depths = [], [], []
        for p in (base @ poses[1], base @ poses[0]):                                  # source t1, target t0
            d = synth.box_room_depth(cam, p, device=dev)
            c = synth.box_room_color(cam, p, d)
            v, n = icp.build_pyramids(d, K, 1)
            maps += [v[0], n[0], rgbd_align.intensity_pyramid(c, 1)[0]]
            colours.append(c.contiguous())
            depths.append(d.reshape(H, W).contiguous())
        vs, ns, i_s, vt, nt, i_t = maps
        pose = torch.eye(4, device=dev)
        scratch6 = torch.empty(lib.rtgs_rgbd_align_scratch_bytes(H, W) // 8, dtype=torch.float64, device=dev)
        scratch8 = torch.empty(lib.rtgs_rgbd_align_exposure_scratch_bytes(H, W) // 8, dtype=torch.float64, device=dev)
        filled = depths[1].clone()
        filled[H // 4:H // 2] = depths[0][H // 4:H // 2]                             # a quarter of the rows count as filled
        fns = {"six_unknowns": lambda: rgbd_align.accumulate(vs, ns, i_s, vt, nt, i_t, K, pose, 0.1, cos, 0.25, 0.05, scratch6),
               "eight_unknowns": lambda: rgbd_align.accumulate_exposure(vs, ns, i_s, vt, nt, i_t, K, pose, 0.1, cos, 0.25, 0.05,
                                                                        0.9, 0.03, scratch8),
               "intensity_pyramid": lambda: rgbd_align.intensity_pyramid(colours[1], 3),
               "target_intensity": lambda: rgbd_align.target_intensity_pyramid(colours[1], colours[0], depths[1], filled, 0.9, 0.03, 3)}
        sums = fns["eight_unknowns"]().cpu().numpy()
        row = {"H": H, "W": W, "calls_per_block": CALLS, "blocks": EXPOSURE_BLOCKS, "geometric_inliers": int(sums[45]),
               "photometric_inliers": int(sums[47])}
        for name, v in _alternating(fns, EXPOSURE_BLOCKS, CALLS).items():
            row[name + "_us_per_call"] = v
        row["note"] = ("per call = host enqueue and the allocation of the results included; the two accumulations are two launches "
                       "each, the two pyramids three")
        rows.append(row)
        print(row, flush=True)
    return rows


def gain_walk(frames, seed=5):
    """(gain, offset) per frame: a bounded random walk inside gain [0.8, 1.25], |offset| <= 0.08; frame 0 is (1, 0)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    g, o, out = 1.0, 0.0, []
    for _ in range(frames):
        out.append((g, o))
        g = float(np.clip(g + rng.normal(0, 0.03), 0.8, 1.25))
        o = float(np.clip(o + rng.normal(0, 0.01), -0.08, 0.08))
    return out


def sequence_exposure(dev, frames):
    import torch
    from rtg_slam_amd import mapping as mp, slam, synth
    cam = synth.REPLICA
    poses = synth.room_tour(frames, seed=21)
    out = {}
    for colour_name, walk in (("clean_colour", None), ("gain_walk", gain_walk(frames))):
        rows = {}
        # the first arm is a short run that is thrown away: it pays for the code objects and the allocator's first blocks
        for name, over, n in (("warm_up", dict(ARMS[3][1]), 30),) + tuple((a, o, frames) for a, o in ARMS):
            args = mp.replica_args(seed=1, rgbd_refine=True, **over)

            def stream():
                for k, c2w in enumerate(poses[:n]):
                    d = synth.box_room_depth(cam, c2w, device=dev)
                    c = synth.box_room_color(cam, c2w, d)
                    if walk is not None:
                        c = (c * walk[k][0] + walk[k][1]).clamp_(0.0, 1.0)
                    torch.cuda.synchronize(dev)
                    yield d.reshape(cam.H, cam.W), c, c2w.numpy()

            _, tracker, rep = slam.run_sequence(cam, stream(), args, dev, capacity=800_000)
            del tracker
            if name == "warm_up":
                continue
            rr = rep["rgbd_refine"]
            rows[name] = {"frames": rep["frames"], "tracker_ms_per_frame": 1e3 * rep["tracking_s_mean"],
                          "mapping_ms_per_frame": 1e3 * rep["mapping_s_mean"], "evaluations_per_frame": rr["host_reads_mean"],
                          "refine_ms_per_frame": rr["ms_mean"], "ate_rmse_m": rep["ate_rmse_m"],
                          "final_translation_error_m": rep["final_translation_error_m"],
                          "exposure": {k: rr[k] for k in ("alpha_mean", "beta_mean", "alpha_min", "alpha_max") if k in rr}}
            print(colour_name, name, rows[name], flush=True)
        out[colour_name] = rows
    out["what"] = (f"slam.run_sequence, {frames} frames of synth.room_tour(seed=21) in the box room at {cam.W}x{cam.H}, clean depth, "
                   "replica_args(seed=1, rgbd_refine=True) from an empty map; arms: plain, + rgbd_refine_exposure, "
                   "+ rgbd_refine_target model, both; gain_walk: the colour of frame k times gain_k plus offset_k, clamped to 0..1, "
                   "a bounded random walk (seed 5) inside gain [0.8, 1.25], |offset| <= 0.08")
    return out


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
    ap.add_argument("--exposure", action="store_true", help="measure the exposure compensation and the model-colour target")
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    opts.out = opts.out or os.path.join(ROOT, "profiles", "r23_rgbd_exposure.json" if opts.exposure else "r22_rgbd_align.json")
    result = {}
    if opts.parent_tree:                                      # first: this process has not opened the GPU yet
        result["bench_ab"] = bench_ab(os.path.abspath(opts.parent_tree), opts.ab_runs)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rgbd_align_check.py needs a GPU; nothing was measured")
    dev = torch.device("cuda", 0)
    result["device"] = torch.cuda.get_device_name(dev)
    result["accumulate"] = time_exposure(dev) if opts.exposure else time_accumulate(dev)
    result["sequence"] = sequence_exposure(dev, opts.frames) if opts.exposure else sequence(dev, opts.frames)
    with open(opts.out, "w") as f:
        json.dump(result, f, indent=1, default=float)
        f.write("\n")
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
