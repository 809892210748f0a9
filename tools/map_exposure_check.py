"""What the mapper's exposure stage (rtg_slam_amd/map_exposure.py) costs and what it changes, on one MI355X -> profiles/r24_map_exposure.json.

    kernels    one fit iteration (two launches), the apply launch and a whole frame's stage (four iterations + apply) beside
               rtgs_add_masks on the same maps at 300x170, 600x340 and 1200x680: device events, a warm-up, then 5 alternating
               blocks, median and range in microseconds per call (host enqueue and the allocation of the results included).
    sequence   slam.run_sequence over FRAMES frames of the box-room tour of tools/rgbd_align_check.py at 1200x680, clean colour
               and that tool's gain walk; arms: rgbd_refine with exposure, with exposure and the model target, both again with
               map_exposure, and map_exposure without rgbd_refine.  Per arm: ATE, tracker and mapping ms per frame, the
               recovered alpha per frame against 1 / gain_k, and the mean absolute colour error of the final map rendered at 10
               of the sequence's poses against the CLEAN colour.
    bench_ab   with --parent-tree DIR (a built checkout of the parent commit): bench.py in alternating fresh processes.

    python tools/map_exposure_check.py [--frames 300] [--parent-tree DIR] [--parts kernels,sequence] [--out profiles/r24_map_exposure.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rgbd_align_check as rac                                                # noqa: E402  (SIZES, _alternating, gain_walk, bench_ab)

CALLS, BLOCKS = 200, 5
EXPOSURE = {"rgbd_refine": True, "rgbd_refine_exposure": True}
ARMS = (("exposure", dict(EXPOSURE)), ("both", dict(EXPOSURE, rgbd_refine_target="model")),
        ("exposure + map_exposure", dict(EXPOSURE, map_exposure=True)),
        ("both + map_exposure", dict(EXPOSURE, rgbd_refine_target="model", map_exposure=True)),
        ("map_exposure", {"map_exposure": True}))


def time_kernels(dev):
    import torch
    from types import SimpleNamespace
    from rtg_slam_amd import map_exposure as me, slam_ops, synth
    rows = []
    pose = synth.look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3)
    for H, W in rac.SIZES:
        s = W / synth.REPLICA.W
        cam = synth.CameraSpec(H, W, synth.REPLICA.fx * s, synth.REPLICA.fy * s, (W - 1) / 2.0, (H - 1) / 2.0)
        d = synth.box_room_depth(cam, pose, device=dev)
        clean = synth.box_room_color(cam, pose, d).contiguous()
        frame = (clean * 1.2 - 0.03).clamp_(0.0, 1.0)
        depth = d.reshape(H, W).contiguous()
        T = torch.zeros(H, W, device=dev)
        index = torch.zeros(H, W, dtype=torch.int32, device=dev)
        render = {"render": clean, "depth": depth, "T_map": T}
        m = me.MapExposure(SimpleNamespace(), dev)
        unit = m.state[:2].clone()

        def whole():
            m.state[:2].copy_(unit)
            m.fit(frame, depth, render)
            m._hist.clear()
            return m.apply(frame)

        fns = {"fit_iteration": lambda: m.fit_iteration(frame, depth, clean, depth, T, 0),
               "apply": lambda: m.apply(frame),
               "frame_stage": whole,
               "add_masks": lambda: slam_ops.add_masks(T, depth, depth, clean, frame, index, 0.5, 0.1, 0.1)}
        whole()
        st = m.state.cpu().numpy()
        row = {"H": H, "W": W, "calls_per_block": CALLS, "blocks": BLOCKS, "alpha": float(st[0]), "beta": float(st[1]),
               "valid_pixels": int(st[me.SUMS_AT + 6]), "bytes_streamed_per_fit_iteration": 36 * H * W}
        for name, v in rac._alternating(fns, BLOCKS, CALLS).items():
            row[name + "_us_per_call"] = v
        row["note"] = ("per call = host enqueue included; fit_iteration is two launches, frame_stage four iterations, a 16-byte state "
                       "reset and the apply launch (11 launches), add_masks one launch")
        rows.append(row)
        print(row, flush=True)
    return rows


def sequence(dev, frames):
    import numpy as np
    import torch
    from rtg_slam_amd import mapping as mp, slam, synth
    cam = synth.REPLICA
    poses = synth.room_tour(frames, seed=21)
    views = list(range(0, frames, max(1, frames // 10)))[:10]
    out = {}
    for colour_name, walk in (("clean_colour", None), ("gain_walk", rac.gain_walk(frames))):
        rows = {}
        # the first arm is a short run that is thrown away: it pays for the code objects and the allocator's first blocks
        for name, over, n in (("warm_up", dict(ARMS[3][1]), 30),) + tuple((a, o, frames) for a, o in ARMS):
            args = mp.replica_args(seed=1, **over)

            def stream():
                for k, c2w in enumerate(poses[:n]):
                    d = synth.box_room_depth(cam, c2w, device=dev)
                    c = synth.box_room_color(cam, c2w, d)
                    if walk is not None:
                        c = (c * walk[k][0] + walk[k][1]).clamp_(0.0, 1.0)
                    torch.cuda.synchronize(dev)
                    yield d.reshape(cam.H, cam.W), c, c2w.numpy()

            mapper, tracker, rep = slam.run_sequence(cam, stream(), args, dev, capacity=800_000)
            del tracker
            if name == "warm_up":
                continue
            errs = []
            for k in views:
                d = synth.box_room_depth(cam, poses[k], device=dev)
                clean = synth.box_room_color(cam, poses[k], d)
                fr = mp.Frame(cam, poses[k], dev, uid=10_000 + k)
                errs.append(float((mapper._render(fr, "all")["render"] - clean).abs().mean()))
            row = {"frames": rep["frames"], "ate_rmse_m": rep["ate_rmse_m"], "tracker_ms_per_frame": 1e3 * rep["tracking_s_mean"],
                   "mapping_ms_per_frame": 1e3 * rep["mapping_s_mean"], "gaussians": rep["gaussians"],
                   "map_colour_error_against_clean": {"mean": sum(errs) / len(errs), "min": min(errs), "max": max(errs),
                                                      "views": views}}
            if "map_exposure" in rep:
                me_rep = rep["map_exposure"]
                alphas = [h[0] for h in mapper.map_exposure.history()]
                want = [1.0 / g for g, _ in (walk or [(1.0, 0.0)] * frames)]
                dev_ = [abs(a - w) for a, w in zip(alphas, want)]
                row["map_exposure"] = {k: me_rep[k] for k in me_rep if k != "options"}
                row["alpha_minus_inverse_gain"] = {"mean_abs": float(np.mean(dev_)), "max_abs": float(np.max(dev_)),
                                                   "mean_abs_of_doing_nothing": float(np.mean([abs(1.0 - w) for w in want]))}
                row["alpha_per_frame"] = [round(a, 4) for a in alphas]
                row["inverse_gain_per_frame"] = [round(w, 4) for w in want]
            del mapper
            rows[name] = row
            print(colour_name, name, {k: v for k, v in row.items() if not k.endswith("_per_frame")}, flush=True)
        out[colour_name] = rows
    out["what"] = (f"slam.run_sequence, {frames} frames of synth.room_tour(seed=21) in the box room at {cam.W}x{cam.H}, clean depth, "
                   "replica_args(seed=1) from an empty map; gain_walk: the colour of frame k times gain_k plus offset_k, clamped to "
                   "0..1, a bounded random walk (seed 5) inside gain [0.8, 1.25], |offset| <= 0.08; the map colour error is the mean "
                   "absolute difference of the final map's render from the clean colour at 10 poses of the sequence")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_map_exposure.json"))
    ap.add_argument("--parts", default="kernels,sequence", help="what to measure now; an existing --out file keeps its other parts")
    opts = ap.parse_args()
    parts = set(opts.parts.split(","))
    result = json.load(open(opts.out)) if os.path.exists(opts.out) else {}
    if opts.parent_tree:                                      # first: this process has not opened the GPU yet
        result["bench_ab"] = rac.bench_ab(os.path.abspath(opts.parent_tree), opts.ab_runs)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("map_exposure_check.py needs a GPU; nothing was measured")
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
