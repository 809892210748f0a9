"""Measures the dataset front end on the GPU host: writes a synthetic Replica-layout dataset (synth.room_tour through the box
room, 1200x680, u16 depth PNGs at scale 6553.5, JPEG colour) into a temporary directory, then runs, alternating, in fresh
processes:

    disk     python -m rtg_slam_amd slam on the dataset (decode pool -> pinned ring -> ingest kernel -> run_sequence)
    memory   run_sequence over the same frames, decoded and ingested onto the GPU before the loop starts

and prints / writes one JSON summary: per run the reference's fps (1 / mean mapping s), tracking + mapping fps, wall frames/s
including I/O (disk), mean I/O wait per frame, decode ms per frame per worker and H2D bytes per frame.

    python tools/dataset_check.py --frames 300 --runs 3 --out profiles/dataset_check.json
    python tools/dataset_check.py gen --data DIR --frames 30        # dataset only (e.g. for a rocprofv3 run of `one`)
    python tools/dataset_check.py one --mode disk --data DIR         # one run, one JSON line
    python tools/dataset_check.py --resolution-scale 2 1 --modes disk  # half size (resized on the device) against full size
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def generate(data: str, n: int, workers: int = 8) -> None:
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from rtg_slam_amd import synth
    cam, dev = synth.REPLICA, torch.device("cuda", 0)
    scene = os.path.join(data, "Replica", "tour")
    os.makedirs(os.path.join(scene, "results"), exist_ok=True)
    poses = synth.room_tour(n, seed=21)

    def write(i, raw, rgb):
        Image.fromarray(raw).save(os.path.join(scene, "results", f"depth{i:06d}.png"))
        Image.fromarray(rgb).save(os.path.join(scene, "results", f"frame{i:06d}.jpg"), quality=95)

    with ThreadPoolExecutor(workers) as pool:
        futs = []
        for i, c2w in enumerate(poses):
            d = synth.box_room_depth(cam, c2w, device=dev)
            c = synth.box_room_color(cam, c2w, d)
            raw = torch.clamp(torch.round(d[..., 0].double() * 6553.5), 0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)
            rgb = torch.clamp(torch.round(c.permute(1, 2, 0).double() * 255), 0, 255).to(torch.uint8).cpu().numpy()
            futs.append(pool.submit(write, i, raw, rgb))
        for f in futs:
            f.result()
    with open(os.path.join(scene, "traj.txt"), "w") as f:
        f.write("".join(" ".join(repr(float(v)) for v in p.numpy().reshape(-1)) + "\n" for p in poses))
    with open(os.path.join(data, "Replica", "cam_params.json"), "w") as f:
        json.dump({"camera": {"w": cam.W, "h": cam.H, "fx": cam.fx, "fy": cam.fy, "cx": cam.cx, "cy": cam.cy, "scale": 6553.5}}, f)


def write_config(data: str, frames: int, resolution_scale: float = 1.0) -> str:
    path = os.path.join(data, "run.yaml")
    with open(path, "w") as f:
        f.write(f'parent: None\ntype: "Replica"\nsource_path: "{os.path.join(data, "Replica", "tour")}"\n'
                f'save_path: "{os.path.join(data, "out")}"\nframe_num: {frames}\nsave_step: 2000\nseed: 1\n'
                f'resolution_scales: [{float(resolution_scale)!r}]\n')
    return path


def one(mode: str, data: str, frames: int, io_workers, resolution_scale: float = 1.0) -> dict:
    import torch
    from rtg_slam_amd import config, datasets
    cfg = write_config(data, frames, resolution_scale)
    if mode == "disk":
        from rtg_slam_amd import __main__ as cli
        argv = ["slam", "--config", cfg, "--overwrite"] + (["--io-workers", str(io_workers)] if io_workers else [])
        rc = cli.main(argv)
        assert rc == 0, rc
        with open(os.path.join(data, "out", "run_report.json")) as f:
            rep = json.load(f)
        info_size = (rep["width"], rep["height"])
    else:
        from rtg_slam_amd.slam import run_sequence
        args = config.load_config(cfg)
        dev = torch.device("cuda", 0)
        info = datasets.load_dataset(args)
        info_size = (info.width, info.height)
        src = datasets.FrameSource(info, dev, io_workers=io_workers)
        frames_gpu = list(src)
        torch.cuda.synchronize(dev)
        st = src.stats()
        _, _, rep = run_sequence(info.camera(), frames_gpu, args, dev, final_global=True, eval_every=int(args.save_step))
        rep.update(io_wait_s_mean=0.0, decode_ms_per_frame=st["decode_ms_per_frame"], io_workers=st["io_workers"],
                   h2d_bytes_per_frame=st["h2d_bytes_per_frame"], wall_fps_including_io=None)
    keep = ("frames", "fps", "fps_tracking_plus_mapping", "tracking_s_mean", "mapping_s_mean", "wall_fps_including_io",
            "io_wait_s_mean", "decode_ms_per_frame", "io_workers", "h2d_bytes_per_frame", "ate_rmse_m", "gaussians")
    return {"mode": mode, "resolution_scale": float(resolution_scale), "image": [info_size[1], info_size[0]],
            **{k: rep.get(k) for k in keep}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", nargs="?", default="all", choices=["all", "gen", "one"])
    ap.add_argument("--data", default=None)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--mode", choices=["disk", "memory"], default="disk")
    ap.add_argument("--io-workers", type=int, default=None)
    ap.add_argument("--resolution-scale", type=float, nargs="+", default=[1.0],
                    help="resolution_scales[0] of the runs; several values alternate (e.g. 2 1: half size against full size)")
    ap.add_argument("--modes", nargs="+", choices=["disk", "memory"], default=["disk", "memory"])
    ap.add_argument("--timeout", type=int, default=240, help="seconds per run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cmd == "gen":
        generate(a.data, a.frames)
        return
    if a.cmd == "one":
        print(json.dumps(one(a.mode, a.data, a.frames, a.io_workers, a.resolution_scale[0])), flush=True)
        return
    data = a.data or tempfile.mkdtemp(prefix="rtgs_dataset_")
    t0 = time.perf_counter()
    generate(data, a.frames)
    print(f"dataset: {a.frames} frames in {time.perf_counter() - t0:.1f} s at {data}", flush=True)
    runs = []
    try:
        for r, scale, mode in ((r, s, m) for r in range(a.runs) for s in a.resolution_scale for m in a.modes):
            cmd = [sys.executable, os.path.abspath(__file__), "one", "--mode", mode, "--data", data, "--frames", str(a.frames),
                   "--resolution-scale", repr(float(scale))]
            if a.io_workers:
                cmd += ["--io-workers", str(a.io_workers)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:
                print(p.stdout[-3000:], p.stderr[-3000:], flush=True)
                raise SystemExit(f"{mode} run {r} at scale {scale} failed with exit status {p.returncode}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            res["run"] = r
            runs.append(res)
            print(json.dumps(res), flush=True)
    finally:
        if a.data is None:
            shutil.rmtree(data, ignore_errors=True)
    summ = {}
    for scale, mode in [(s, m) for s in a.resolution_scale for m in a.modes]:
        rs = [x for x in runs if x["mode"] == mode and x["resolution_scale"] == float(scale)]
        fps = [x["fps"] for x in rs]
        name = mode if float(scale) == 1.0 else f"{mode}@scale{float(scale):g}"
        summ[name] = {"image": rs[0]["image"], "fps": fps, "fps_median": statistics.median(fps), "fps_spread": max(fps) - min(fps),
                      "fps_tracking_plus_mapping": [x["fps_tracking_plus_mapping"] for x in rs],
                      "tracking_ms_mean": [round(1e3 * x["tracking_s_mean"], 4) for x in rs],
                      "mapping_ms_mean": [round(1e3 * x["mapping_s_mean"], 4) for x in rs],
                      "wall_fps_including_io": [x["wall_fps_including_io"] for x in rs],
                      "io_wait_ms_mean": [round(1e3 * x["io_wait_s_mean"], 4) for x in rs],
                      "decode_ms_per_frame_per_worker": [round(x["decode_ms_per_frame"], 3) for x in rs],
                      "io_workers": rs[0]["io_workers"], "h2d_bytes_per_frame": rs[0]["h2d_bytes_per_frame"]}
    out = {"frames": a.frames, "image": [680, 1200], "runs": runs, "summary": summ}
    print(json.dumps(out["summary"], indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
