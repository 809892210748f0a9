"""Times the stable cloud's densification (pcd_densify) and prints one JSON line (also written to OUT when given):
  * the rtgs_densify_discs kernel alone, with device events after warm-up, at P = 300 k and 1.2 M stable Gaussians
    (K = 150: densify(1, 30, 5)), into a preallocated float64 buffer; the rate counts the 48 B written per point;
  * at P = 300 k, separately: the device-to-host copy of the whole result into pinned memory, the file write of it
    (io_formats.PointCloudPlyWriter, header + records), and metric's read of the file (load_point_cloud_ply), its upload and
    the subsample to 1 M rows (evaluation.subsample, as eval_pcd draws it).
The map is random (scales with ties, unit quaternions); the file goes to a temporary directory and is removed.
python tools/densify_check.py [OUT] [reps = 20]"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtg_slam_amd import evaluation as ev, io_formats as iof, slam_ops as so   # noqa: E402


def random_map(P, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(P, 3, generator=g) * 3.0
    s = torch.exp(torch.randn(P, 3, generator=g) * 0.8 - 3.0)
    s[::3, 1] = s[::3, 0]
    q = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=1)
    return xyz.to(dev), s.to(dev), q.to(dev)


def event_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "reps": reps}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda", 0)
    sigma, C, L = 1, 30, 5
    K = sigma * C * L
    cos, sin = (t.to(dev) for t in so.densify_theta(C, torch.Generator().manual_seed(0)))
    res = {"device": torch.cuda.get_device_name(dev), "sigma_circle_levels": [sigma, C, L], "bytes_per_point": 48}
    for P in (300_000, 1_200_000):
        xyz, s, q = random_map(P, dev)
        buf = torch.empty(P * K, 6, dtype=torch.float64, device=dev)
        t = event_ms(lambda: so.densify_discs(xyz, s, q, cos, sin, sigma, L, out=buf), reps)
        nbytes = P * K * 48
        t["GB_written"] = round(nbytes / 1e9, 3)
        t["TB_per_s_at_median"] = round(nbytes / (t["median_ms"] * 1e-3) / 1e12, 3)
        res[f"kernel_P{P}"] = t
        if P != 300_000:
            del buf, xyz, s, q
            continue
        host = torch.empty(P * K, 6, dtype=torch.float64, pin_memory=True)
        d2h = event_ms(lambda: host.copy_(buf, non_blocking=True), max(3, reps // 4), warmup=1)
        d2h["GB_per_s_at_median"] = round(nbytes / (d2h["median_ms"] * 1e-3) / 1e9, 2)
        res["d2h_pinned_P300000"] = d2h
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "pcd_densify.ply")
            t0 = time.perf_counter()
            with iof.PointCloudPlyWriter(path, P * K) as w:
                w.write(host.numpy())
            os.sync()
            t_write = time.perf_counter() - t0
            size = os.path.getsize(path)
            res["file_write_P300000"] = {"s": round(t_write, 3), "bytes": size, "GB_per_s": round(size / t_write / 1e9, 2),
                                         "includes": "write() of the pinned buffer + os.sync()"}
            t0 = time.perf_counter()
            pts, nrm = iof.load_point_cloud_ply(path)
            t_read = time.perf_counter() - t0
            assert pts.shape == (P * K, 3) and np.array_equal(pts, host[:, :3].numpy())
            del nrm
            t0 = time.perf_counter()
            rec = torch.from_numpy(pts).to(device=dev, dtype=torch.float32)
            torch.cuda.synchronize()
            t_up = time.perf_counter() - t0
            t0 = time.perf_counter()
            sub = ev.subsample(rec, 1_000_000)
            torch.cuda.synchronize()
            t_sub = time.perf_counter() - t0
            assert sub.shape == (1_000_000, 3)
            res["metric_read_P300000"] = {"load_point_cloud_ply_s": round(t_read, 3), "upload_float32_s": round(t_up, 3),
                                          "subsample_to_1M_s": round(t_sub, 3),
                                          "note": "the file was just written: the read may be served by the page cache"}
        del buf, host, xyz, s, q
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
