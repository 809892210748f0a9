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

With --channels the subject is `map_exposure_channels: rgb` (csrc/white_balance.hip) -> profiles/r25_white_balance.json:
    kernels    the same three figures for the grey and the rgb stage side by side, in the same alternating blocks.
    sequence   the tour under three INDEPENDENT gain walks, one per colour channel (seeds 5, 6, 7); arms: option off, grey, rgb.
               Per arm: ATE, map colour error against the clean colour, Gaussians, mapping ms per frame.  Then the grey arm's map
               is scored over every tenth frame at the tracked poses with evaluate_sequence(exposure_aware=True), what `metric
               --exposure-aware` runs: plain against exposure-aware PSNR.

    python tools/map_exposure_check.py [--channels] [--frames 300] [--parent-tree DIR] [--parts kernels,sequence] [--out FILE]"""
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


def time_channel_kernels(dev):
    """time_kernels for the grey and the rgb stage in the same alternating blocks."""
    import torch
    from types import SimpleNamespace
    from rtg_slam_amd import map_exposure as me, synth
    rows = []
    pose = synth.look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3)
    tint = torch.tensor([1.25, 1.1, 0.95], device=dev).reshape(3, 1, 1)
    for H, W in rac.SIZES:
        s = W / synth.REPLICA.W
        cam = synth.CameraSpec(H, W, synth.REPLICA.fx * s, synth.REPLICA.fy * s, (W - 1) / 2.0, (H - 1) / 2.0)
        d = synth.box_room_depth(cam, pose, device=dev)
        clean = synth.box_room_color(cam, pose, d).contiguous()
        frame = (clean * tint - 0.03).clamp_(0.0, 1.0)
        depth = d.reshape(H, W).contiguous()
        T = torch.zeros(H, W, device=dev)
        render = {"render": clean, "depth": depth, "T_map": T}
        fns, stages = {}, {}
        for ch in me.CHANNELS:
            m = stages[ch] = me.MapExposure(SimpleNamespace(map_exposure_channels=ch), dev)
            unit = m.state.clone()

            def whole(m=m, unit=unit):
                m.state.copy_(unit)
                m.fit(frame, depth, render)
                m._hist.clear()
                return m.apply(frame)

            fns.update({f"fit_iteration_{ch}": lambda m=m: m.fit_iteration(frame, depth, clean, depth, T, 0),
                        f"apply_{ch}": lambda m=m: m.apply(frame), f"frame_stage_{ch}": whole})
            whole()
        st = stages["rgb"].state.cpu().numpy()
        row = {"H": H, "W": W, "calls_per_block": CALLS, "blocks": BLOCKS, "chunks": -(-H * W // 1024),
               "alpha_rgb": [float(st[me.WB_REG * c]) for c in (1, 2, 3)], "alpha_grey": float(stages["grey"].state[0]),
               "valid_pixels": int(st[me.WB_SUMS_AT + me.WB_VALID]), "bytes_streamed_per_fit_iteration": 36 * H * W}
        for name, v in rac._alternating(fns, BLOCKS, CALLS).items():
            row[name + "_us_per_call"] = v
        row["note"] = ("per call = host enqueue included; fit_iteration is two launches, frame_stage four iterations, a state reset "
                       "and the apply launch (11 launches) in both modes; both modes stream the same 36 bytes per pixel")
        rows.append(row)
        print(row, flush=True)
    return rows


def channel_walk(frames):
    """Per frame (gains[3], offsets[3]): three independent walks of rgbd_align_check.gain_walk, seeds 5, 6, 7."""
    walks = [rac.gain_walk(frames, seed=5 + c) for c in range(3)]
    return [([w[k][0] for w in walks], [w[k][1] for w in walks]) for k in range(frames)]


def sequence_channels(dev, frames):
    import torch
    from rtg_slam_amd import evaluation, mapping as mp, slam, synth
    cam = synth.REPLICA
    poses = synth.room_tour(frames, seed=21)
    views = list(range(0, frames, max(1, frames // 10)))[:10]
    walk = [(torch.tensor(g, device=dev).reshape(3, 1, 1), torch.tensor(o, device=dev).reshape(3, 1, 1))
            for g, o in channel_walk(frames)]
    arms = (("warm_up", {"map_exposure": True, "map_exposure_channels": "rgb"}, 30), ("off", {}, frames),
            ("grey", {"map_exposure": True}, frames), ("rgb", {"map_exposure": True, "map_exposure_channels": "rgb"}, frames))

    def stream(ids):
        for k in ids:
            d = synth.box_room_depth(cam, poses[k], device=dev)
            c = (synth.box_room_color(cam, poses[k], d) * walk[k][0] + walk[k][1]).clamp_(0.0, 1.0)
            torch.cuda.synchronize(dev)
            yield d.reshape(cam.H, cam.W), c, poses[k].numpy()

    rows = {}
    for name, over, n in arms:
        args = mp.replica_args(seed=1, **over)
        mapper, tracker, rep = slam.run_sequence(cam, stream(range(n)), args, dev, capacity=800_000)
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
               "map_colour_error_against_clean": {"mean": sum(errs) / len(errs), "min": min(errs), "max": max(errs), "views": views}}
        if "map_exposure" in rep:
            row["map_exposure"] = {k: v for k, v in rep["map_exposure"].items() if k != "options"}
        if name == "grey":                                    # what `metric --exposure-aware` runs, on every tenth frame
            ids = list(range(0, frames, 10))
            res = evaluation.evaluate_sequence(mapper, cam, stream(ids), poses=[tracker.pose_es[k] for k in ids], args=args,
                                               exposure_aware=True)
            row["exposure_aware"] = dict(res["exposure_mean"], frames=len(ids), device_s=res["exposure_seconds"],
                                         psnr_gain_db=res["exposure_mean"]["psnr_ea"] - res["exposure_mean"]["psnr"])
        del mapper, tracker
        rows[name] = row
        print(name, row, flush=True)
    rows["what"] = (f"slam.run_sequence, {frames} frames of synth.room_tour(seed=21) in the box room at {cam.W}x{cam.H}, clean depth, "
                    "replica_args(seed=1) from an empty map, ICP tracking; channel c of frame k times gain_kc plus offset_kc, clamped "
                    "to 0..1, three independent bounded random walks (seeds 5, 6, 7) inside gain [0.8, 1.25], |offset| <= 0.08; the map "
                    "colour error is the mean absolute difference of the final map's render from the clean colour at 10 poses")
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
    ap.add_argument("--channels", action="store_true", help="measure map_exposure_channels: rgb beside grey (-> r25_white_balance.json)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="kernels,sequence", help="what to measure now; an existing --out file keeps its other parts")
    opts = ap.parse_args()
    if opts.out is None:
        opts.out = os.path.join(ROOT, "profiles", "r25_white_balance.json" if opts.channels else "r24_map_exposure.json")
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
        result["kernels"] = (time_channel_kernels if opts.channels else time_kernels)(dev)
    if "sequence" in parts:
        result["sequence"] = (sequence_channels if opts.channels else sequence)(dev, opts.frames)
    with open(opts.out, "w") as f:
        json.dump(result, f, indent=1, default=float)
        f.write("\n")
    print("wrote", opts.out)


if __name__ == "__main__":
    main()
