"""Times the mesh renderer (evaluation.MeshRenderer, csrc/mesh_render.hip) on the device and prints one JSON line (also written
to OUT when given).  1200 x 680, the Replica camera inside the box room at poses of synth.room_tour, three meshes:
  * the room fused at 2 cm and at 1 cm voxels as tools/mesh_check.py fuses it (faces of a few pixels),
  * the 10 cm wall grid (visibility_reference.box_grid: faces that span thousands of pixels).
Per mesh: the per-render time of the thread-only form (small_max = 2^31 - 1: no face is queued) and of the two-path form at
several small_max, blocks of every form alternating in one run; the share of faces the two-path form queues (the queue's
counter, read back after a render); the bytes a render must move - 12 B per face, 12 B per vertex, 16 B per pixel - over the
median time.  Then the box-room end-to-end case of tools/mesh_check.py with cull_unseen on: what it removes.
Timing: device events around `reps` renders, after a warm-up, in `blocks` blocks; the median block and the spread of the
blocks are reported.  python tools/mesh_render_check.py [OUT] [reps = 10] [blocks = 5]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtg_slam_amd import evaluation, meshing, synth   # noqa: E402
from tools.mesh_check import alternating_blocks_ms, _finish   # noqa: E402

THREAD_ONLY = 2 ** 31 - 1
SMALL_MAX = (THREAD_ONLY, 0, 4, 8, 16, 32, 64, 256, 1024)


def _queued(renderer, cam):
    """The number of faces the last render queued: the counter behind the H * W keys of the scratch."""
    return int(renderer._scratch[cam.H * cam.W].item()) & 0xFFFFFFFF


def render_leg(name, v, f, cam, poses, reps, blocks):
    renderers = {("thread_only" if s == THREAD_ONLY else f"small_max_{s}"): evaluation.MeshRenderer(v, f, cam, small_max=s) for s in SMALL_MAX}
    first = next(iter(renderers.values()))
    V, F = int(first.vertices.shape[0]), int(first.faces.shape[0])
    moved = 12 * F + 12 * V + 16 * cam.H * cam.W
    entry = {"V": V, "F": F, "bytes_moved_lower_bound": moved}
    ref = [first.render(p) for p in poses]
    same, queued = True, {}
    for key, r in renderers.items():
        n = []
        for p, (d0, f0) in zip(poses, ref):
            d, fm = r.render(p)
            same = same and torch.equal(d, d0) and torch.equal(fm, f0)
            n.append(_queued(r, cam))
        queued[key] = round(float(np.mean(n)) / max(F, 1), 6)
    entry["all_forms_render_the_same_picture"] = bool(same)
    entry["covered_share_mean"] = round(float(np.mean([float((d > 0).float().mean()) for d, _ in ref])), 4)
    entry["queued_share_of_faces"] = queued
    call = lambda r: (lambda i: r.render(poses[i % len(poses)]))
    for r in renderers.values():
        r.seconds                                                                  # forget the events so far
    t = alternating_blocks_ms({k: call(r) for k, r in renderers.items()}, reps, blocks)
    for k in t:
        t[k]["TB_per_s_of_moved_bytes_at_median"] = round(moved / (t[k]["median_ms"] * 1e-3) / 1e12, 4)
        t[k]["over_thread_only"] = round(t[k]["median_ms"] / t["thread_only"]["median_ms"], 3)
    entry["render_call"] = t
    # the four launches alone: the renderer's own event pair around every render of the blocks above (warm-up dropped),
    # summed per block of reps renders as the blocks were run
    torch.cuda.synchronize()
    k_ms = {}
    for k, r in renderers.items():
        ms = np.array([a.elapsed_time(b) for a, b in r._events][-reps * blocks:]).reshape(blocks, reps).mean(axis=1)
        k_ms[k] = {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4),
                   "TB_per_s_of_moved_bytes_at_median": round(moved / (float(np.median(ms)) * 1e-3) / 1e12, 4)}
    for k in k_ms:
        k_ms[k]["over_thread_only"] = round(k_ms[k]["median_ms"] / k_ms["thread_only"]["median_ms"], 3)
    entry["kernels"] = k_ms
    print(name, json.dumps(entry), flush=True)
    return entry


def main():
    argv = sys.argv[1:]
    out_path = argv[0] if len(argv) > 0 else None
    reps = int(argv[1]) if len(argv) > 1 else 10
    blocks = int(argv[2]) if len(argv) > 2 else 5
    dev = torch.device("cuda", 0)
    cam = synth.REPLICA
    res = {"device": torch.cuda.get_device_name(dev), "camera": [cam.W, cam.H],
           "timing": "render_call: device events around reps .render calls (the host's 4 x 4 inverse, two output tensors and the "
                     "four launches: where the host is slower than the kernels this is the host's time), blocks of all forms "
                     "alternating, after a warm-up of 3 renders per form; kernels: the event pair around the four launches of "
                     "each of those renders, averaged per block",
           "yardsticks": {"extract_mesh_ms": {"2cm": 1.6, "1cm": 7.0}, "frame_decode_ms": 6.3, "streaming_TB_per_s": [3.9, 5.3]}}
    tour = [p for p in synth.room_tour(reps * 40, seed=3)[::40]]
    frames = []
    for p in tour:
        d = synth.box_room_depth(cam, p, device=dev)
        frames.append((d.reshape(cam.H, cam.W).contiguous(), synth.box_room_color(cam, p, d), p.numpy()))
    poses = [p.numpy() for p in tour]
    half = (2.5, 1.5, 3.0)
    lo, hi = [-h - 0.1 for h in half], [h + 0.1 for h in half]
    for voxel in (0.02, 0.01):
        vol = meshing.TsdfVolume(lo, hi, voxel, device=dev)
        for d, c, p in frames:
            vol.integrate(d, c, cam, p)
        v, f, _ = vol.extract_mesh()
        del vol
        torch.cuda.empty_cache()
        res[f"room_voxel_{voxel:g}"] = render_leg(f"room_voxel_{voxel:g}", v, f, cam, poses, reps, blocks)
        del v, f
    from tests import visibility_reference as vr
    gv, gf = vr.box_grid(vr.ROOM_HALF)
    res["wall_grid_10cm"] = render_leg("wall_grid_10cm", gv, gf, cam, poses, reps, blocks)

    # the end-to-end case of tools/mesh_check.py (tests/test_mesh_gpu.py), with the unseen surface removed
    from tests import tsdf_reference as tr
    bcam, bframes, blo, bhi, bvoxel = tr.box_room_case()
    stream = [(d.to(dev), c.to(dev), p) for d, c, p in bframes]
    _, _, _, report = meshing.mesh_from_map(None, bcam, None, iter(stream), voxel=bvoxel, depth_source="sensor", bounds=(blo, bhi),
                                            device=dev, cull_unseen=True)
    res["box_room_sensor_2cm_cull_unseen"] = {"camera": [bcam.W, bcam.H], "report": report}
    res["default_small_max"] = evaluation.MESH_RENDER_SMALL_MAX
    _finish(res, out_path)


if __name__ == "__main__":
    main()
