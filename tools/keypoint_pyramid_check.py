"""Times the keypoint pyramid and the keypoint votes on the device: python tools/keypoint_pyramid_check.py [--out FILE.json]

    features   keypoints.detect_and_describe per frame at 1, 3 and 5 levels, at 320 x 240, 600 x 340 and 1200 x 680, the settings
               alternating within every block (device events around each call: the launches and the small copy to the host)
    votes      one match launch and one rtgs_keypoint_votes launch of a lost frame against M = 71, 500 and 2 000 keyframes
               (keypoints.vote_pairs, 3 levels, 320 x 240), and the vote launch alone
    search     LoopCloser._keypoint_search's vote and RANSAC stages over all pairs of M <= 500 keyframes, min_gap 10 (wall clock)

The frames are views of the textured box room; the M keyframes repeat 71 views of one turn, which costs what M different ones
cost.  A warm-up, then the median and the range of 5 blocks."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtg_slam_amd import keypoints as kp, synth  # noqa: E402
from rtg_slam_amd.rgbd_align import se3_exp  # noqa: E402

DEV = torch.device("cuda", 0)
BLOCKS, REPEATS = 5, 10
SEARCH_MAX = 500                                                    # keyframes up to which the whole search is timed (it is quadratic)


def view(cam, yaw_deg):
    T = se3_exp([0.0, np.deg2rad(yaw_deg), 0.0, 0.0, 0.0, 0.0])
    T[:3, 3] = (0.15, -0.1, 0.2)
    p = torch.from_numpy(T)
    d = synth.box_room_depth(cam, p)
    return synth.box_room_texture_color(cam, p, d).to(DEV), d.to(DEV).reshape(1, cam.H, cam.W)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def features():
    out = {}
    for W, H in ((320, 240), (600, 340), (1200, 680)):
        cam = synth.CameraSpec(H, W, W / 2.0, W / 2.0, (W - 1) / 2.0, (H - 1) / 2.0)
        K = np.array([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1.0]])
        c, d = view(cam, 20.0)
        cfgs = {L: kp.config(levels=L) for L in (1, 3, 5)}
        n = {L: int(len(kp.detect_and_describe(c, d, K, cfg)["x"])) for L, cfg in cfgs.items()}      # the warm-up
        blocks = {L: [] for L in cfgs}
        for _ in range(BLOCKS):
            ms = {L: [] for L in cfgs}
            for _ in range(REPEATS):
                for L, cfg in cfgs.items():                          # alternating
                    ms[L].append(timed(lambda: kp.detect_and_describe(c, d, K, cfg)))
            for L in cfgs:
                blocks[L].append(float(np.median(ms[L])))
        out[f"{W}x{H}"] = {f"levels_{L}": dict(stats(blocks[L]), keypoints=n[L]) for L in cfgs}
        print(f"{W}x{H}", out[f"{W}x{H}"], flush=True)
    return out


def votes_and_search():
    from types import SimpleNamespace
    from rtg_slam_amd import loop_closure as lc
    cam = synth.CameraSpec(240, 320, 160.0, 160.0, 159.5, 119.5)
    K = np.array([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1.0]])
    cfg = kp.config(levels=3)
    base = [kp.detect_and_describe(*view(cam, 360.0 * k / 71), K, cfg) for k in range(71)]
    frame = kp.detect_and_describe(*view(cam, 33.0), K, cfg)
    out = {}
    for M in (71, 500, 2000):
        feats = {a: base[a % 71] for a in range(M)}
        feats["frame"] = frame
        pairs = [(a, "frame") for a in range(M)]
        kp.vote_pairs(feats, pairs, cfg)
        both, alone = [], []
        for _ in range(BLOCKS):
            both.append(float(np.median([timed(lambda: kp.vote_pairs(feats, pairs, cfg)) for _ in range(REPEATS)])))
            matches, where = kp.match_pairs_device(feats, [q for a, b in pairs for q in ((b, a), (a, b))])
            table = [(where[2 * n][0], where[2 * n][1], where[2 * n + 1][0], where[2 * n + 1][1]) for n in range(M)]
            alone.append(float(np.median([timed(lambda: kp.keypoint_votes(matches, table, DEV, cfg.max_hamming, cfg.ratio)) for _ in range(REPEATS)])))
        out[f"keyframes_{M}"] = {"lost_frame_match_and_votes": stats(both), "vote_launch": stats(alone)}
        if M > SEARCH_MAX:
            print(M, out[f"keyframes_{M}"], flush=True)
            continue
        closer = lc.LoopCloser.__new__(lc.LoopCloser)                 # the search's vote stage alone: no refiner, no mapper
        closer.cfg = SimpleNamespace(min_gap=10, max_per_keyframe=2)
        closer.keypoints = SimpleNamespace(cfg=cfg, shortlist=3)
        mapper = SimpleNamespace(device=DEV, keyframe_list=[SimpleNamespace(K=K)], keymap_list=[{"color_chw": None, "depth_chw": None}] * M)
        real = kp.detect_and_describe
        it = iter(range(M))
        kp.detect_and_describe = lambda *a, **k: base[next(it) % 71]   # the features are timed above
        try:
            rep = {}
            t0 = time.perf_counter()
            found = closer._keypoint_search(mapper, [np.eye(4)] * M, rep)
            wall = time.perf_counter() - t0
        finally:
            kp.detect_and_describe = real
        ks = rep["keypoint_search"]
        out[f"keyframes_{M}"].update({"search": {"pairs_voted": ks["pairs_voted"], "chunks": ks["chunks"], "shortlisted": ks["shortlisted"],
                                            "candidates": len(found), "votes_s": ks["seconds"]["votes"], "ransac_s": ks["seconds"]["ransac"],
                                            "wall_s": wall}})
        print(M, out[f"keyframes_{M}"], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-search", action="store_true")
    o = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "blocks": BLOCKS, "repeats_per_block": REPEATS, "features": features()}
    if not o.skip_search:
        res["votes_and_search"] = votes_and_search()
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
