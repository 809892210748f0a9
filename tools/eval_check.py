"""Times the evaluation kernels with device events after warm-up and prints one JSON line:
  * picture metrics (rtgs_eval_picture incl. MS-SSIM) at 1200 x 680 on a rasterizer render of a synthetic map;
  * the kernels alone (picture_metrics: the result left on the device) and eval_picture (plus the one read of the vector);
  * reconstruction metrics at N x N points, both directions, the two search-structure builds included (eval_pcd).
python tools/eval_check.py [N = 1000000] [reps = 20]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtg_slam_amd import evaluation as ev, io_formats as iof, mapping as mp, synth   # noqa: E402
from rtg_slam_amd.render import Renderer   # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4)}


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda", 0)
    cam = synth.REPLICA
    c2w = torch.eye(4, dtype=torch.float64)
    gs = {k: v.to(dev) for k, v in synth.surface_gaussians(290_000, cam, seed=7).items()}
    with torch.no_grad():
        out = Renderer(mp.replica_args()).render(mp.Frame(cam, c2w.numpy(), dev), gs)
    gt_depth = synth.box_room_depth(cam, c2w).reshape(cam.H, cam.W).to(dev)
    gt_color = synth.box_room_color(cam, c2w, gt_depth.cpu()[..., None]).to(dev)
    args = (out["render"], gt_color, out["depth"], gt_depth, out["depth_index_map"], 0.3, 5.0)
    pic_kernels = timed(lambda: ev.picture_metrics(*args), reps)
    pic_no_ms = timed(lambda: ev.picture_metrics(*args, with_ms_ssim=False), reps)
    pic_call = timed(lambda: ev.eval_picture(out, gt_color, gt_depth, 0.3, 5.0), reps)
    metrics = ev.eval_picture(out, gt_color, gt_depth, 0.3, 5.0)

    # N GT points on the room's walls, N reconstruction points: the map's centres style (noisy, one wall short)
    v = np.array([[x, y, z] for x in (-2.5, 2.5) for y in (-1.5, 1.5) for z in (-3.0, 3.0)], dtype=np.float64)
    q = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]])
    f = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])
    gt = torch.tensor(iof.sample_mesh_surface(v, f, N, seed=1)[0], dtype=torch.float32, device=dev)
    rec = torch.tensor(iof.sample_mesh_surface(v, f[2:], N, seed=2)[0], dtype=torch.float32, device=dev)
    rec = rec + 0.005 * torch.randn(N, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    pcd = timed(lambda: ev.eval_pcd(rec, gt, (0.01, 0.03, 0.05)), max(3, reps // 4))
    pcd_res = ev.eval_pcd(rec, gt, (0.01, 0.03, 0.05))
    print(json.dumps({
        "device": torch.cuda.get_device_name(dev),
        "picture_1200x680": {"kernels_ms_ssim": pic_kernels, "kernels_no_ms_ssim": pic_no_ms, "eval_picture_call": pic_call,
                             "metrics": metrics},
        f"pcd_{N}x{N}": {"eval_pcd_call": pcd, "metrics": pcd_res},
    }))


if __name__ == "__main__":
    main()
