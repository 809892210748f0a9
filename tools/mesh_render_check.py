"""Times the mesh renderer (evaluation.MeshRenderer, csrc/mesh_render.hip) on the device and prints one JSON line (also written
to OUT when given).  1200 x 680, the Replica camera inside the box room at poses of synth.room_tour, three meshes:
  * the room fused at 2 cm and at 1 cm voxels as tools/mesh_check.py fuses it (faces of a few pixels),
  * the 10 cm wall grid (visibility_reference.box_grid: faces that span thousands of pixels).
Per mesh: the per-render time of the thread-only form (small_max = 2^31 - 1: no face is queued) and of the two-path form at
several small_max, blocks of every form alternating in one run; the share of faces the two-path form queues (the queue's
counter, read back after a render); the bytes a render must move - 12 B per face, 12 B per vertex, 16 B per pixel - over the
median time.  Then the box-room end-to-end case of tools/mesh_check.py with cull_unseen on: what it removes.
Timing: device events around `reps` renders, after a warm-up, in `blocks` blocks; the median block and the spread of the
blocks are reported.  python tools/mesh_render_check.py [OUT] [reps = 10] [blocks = 5]
With --color (profiles/r21_mesh_shade.json) it times the colour pass instead: the two rooms in their vertex colours, their 10 %
decimations in vertex colours and with the atlas baked at half the voxel - rtgs_mesh_shade alone per source, the four-launch
render beside it, the whole render_color calls, the counted bytes, and the PSNR of the colour renders against the frames.
--parent-lib=PATH names a build of the library from the parent commit: its rtgs_mesh_render then alternates with this build's
on the same inputs, and the pictures of both are hashed."""
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


def _shade_call(lib, r, cam, m, face, color, source):
    """One rtgs_mesh_shade launch of renderer r's mesh on a face map already rendered (the colour pass alone)."""
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(None)
    vertex = source == "vertex"
    bg = (C.c_float * 3)(0.0, 0.0, 0.0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fx, fy, cx, cy = (float(np.float32(k)) for k in (cam.fx, cam.fy, cam.cx, cam.cy))
    Ht, Wt = (1, 1) if vertex else (int(r.texture.shape[0]), int(r.texture.shape[1]))
    rc = lib.rtgs_mesh_shade(p(r.vertices), int(r.vertices.shape[0]), p(r.faces), int(r.faces.shape[0]), p(face), cam.H, cam.W, fx, fy, cx, cy,
                             m, r.near, p(r.colors) if vertex else null, null if vertex else p(r.uv), null if vertex else p(r.texture),
                             Ht, Wt, bg, p(color), stream)
    assert rc == 0, rc
    return color


def _parent_render(path):
    """rtgs_mesh_render of another build of the library (the parent commit's), with this build's argument types."""
    import ctypes as C
    from rtg_slam_amd import _lib
    lib = C.CDLL(path)
    lib.rtgs_mesh_render.restype, lib.rtgs_mesh_render.argtypes = _lib.load().rtgs_mesh_render.restype, _lib.load().rtgs_mesh_render.argtypes
    return lib.rtgs_mesh_render


def _picture_hash(*tensors):
    import hashlib
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def color_leg(name, r, cam, frames, reps, blocks, sources, parent=None):
    """The colour pass of renderer r alone, per source, beside its four-launch render; the counted bytes; the PSNR of the colour
    renders against the frames; with `parent` (rtgs_mesh_render of the parent commit's library) both builds' render alternating."""
    import ctypes as C
    from rtg_slam_amd import _lib
    lib = _lib.load()
    n = len(frames)
    poses = [p for _, _, p in frames]
    views = [r._view(p)[0] for p in poses]
    maps = [r.render(p) for p in poses]
    V, F = int(r.vertices.shape[0]), int(r.faces.shape[0])
    pixels = cam.H * cam.W
    entry = {"V": V, "F": F, "covered_share_mean": round(float(np.mean([float((d > 0).float().mean()) for d, _ in maps])), 4),
             "bytes_per_pixel": {"face_map_read": 4, "out_written": 12,
                                 "gathers_vertex": "3 x 4 B corner indices + 3 x 12 B corner positions + 3 x 12 B corner colours = 84 B",
                                 "gathers_texture": "3 x 4 B indices + 3 x 12 B positions + 24 B uv + 4 texels x 3 B = 84 B"},
             "bytes_streamed": 16 * pixels}
    if "texture" in sources:
        entry["atlas"] = [int(r.texture.shape[1]), int(r.texture.shape[0])]
    color = torch.empty(3, cam.H, cam.W, dtype=torch.float32, device=r.device)
    fns = {"mesh_render": lambda i: r.render(poses[i % n])}
    for s in sources:
        fns[f"shade_{s}"] = (lambda s: lambda i: _shade_call(lib, r, cam, views[i % n], maps[i % n][1], color, s))(s)
        fns[f"render_color_{s}"] = (lambda s: lambda i: r.render_color(poses[i % n], s))(s)
    if parent is not None:
        depth = torch.empty(cam.H, cam.W, dtype=torch.float32, device=r.device)
        face = torch.empty(cam.H, cam.W, dtype=torch.int32, device=r.device)
        p = lambda t: C.c_void_p(t.data_ptr())
        fx, fy, cx, cy = (float(np.float32(k)) for k in (cam.fx, cam.fy, cam.cx, cam.cy))

        def raw(fn):
            def call(i):
                rc = fn(p(r.vertices), V, p(r.faces), F, cam.H, cam.W, fx, fy, cx, cy, views[i % n], r.near, r.small_max, p(r._scratch),
                        p(depth), p(face), C.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 0, rc
            return call
        hashes = {}
        for key, fn in (("this", lib.rtgs_mesh_render), ("parent", parent)):
            hashes[key] = []
            for i in range(n):
                raw(fn)(i)
                hashes[key].append(_picture_hash(depth, face))
            fns[f"rtgs_mesh_render_{key}"] = raw(fn)
        entry["picture_hashes"] = hashes["this"]
        entry["parent_pictures_identical"] = hashes["this"] == hashes["parent"]
    timed = alternating_blocks_ms(fns, reps, blocks)
    for s in sources:
        ms = timed[f"shade_{s}"]["median_ms"]
        timed[f"shade_{s}"]["TB_per_s_of_streamed_bytes_at_median"] = round(16 * pixels / (ms * 1e-3) / 1e12, 3)
        timed[f"shade_{s}"]["over_mesh_render"] = round(ms / timed["mesh_render"]["median_ms"], 3)
    entry["times"] = timed
    quality = {}
    for s in sources:
        rows = [evaluation.mesh_color_metrics(r.render_color(p, s)[0], col, maps[i][1]) for i, (_, col, p) in enumerate(frames)]
        quality[s] = {k: round(float(np.mean([row[k] for row in rows])), 5) for k in rows[0]}
    entry["against_the_frames"] = quality
    print(name, json.dumps(entry), flush=True)
    return entry


def color_main(out_path, reps, blocks, parent_path):
    """--color: the room fused at 2 cm and 1 cm in its vertex colours, and its 10 % decimation in vertex colours and with the atlas
    baked at half the voxel from the same frames."""
    from rtg_slam_amd import mesh_ops
    dev = torch.device("cuda", 0)
    cam = synth.REPLICA
    parent = _parent_render(parent_path) if parent_path else None
    res = {"device": torch.cuda.get_device_name(dev), "camera": [cam.W, cam.H], "parent_library": bool(parent_path),
           "timing": "device events around reps calls per block, blocks of every form alternating, after a warm-up of 3 calls per "
                     "form.  mesh_render / render_color_*: the Python calls (where the host is slower than the kernels this is the "
                     "host's time); shade_*: rtgs_mesh_shade alone through ctypes on face maps rendered before; rtgs_mesh_render_this "
                     "/ _parent: the four-launch call alone through ctypes, this build and the parent commit's",
           "yardsticks": {"mesh_render_kernels_ms_r15": {"2cm": 0.085, "1cm": 0.099}}}
    tour = [p for p in synth.room_tour(reps * 40, seed=3)[::40]]
    frames = []
    for p in tour:
        d = synth.box_room_depth(cam, p, device=dev)
        frames.append((d.reshape(cam.H, cam.W).contiguous(), synth.box_room_color(cam, p, d), p.numpy()))
    half = (2.5, 1.5, 3.0)
    lo, hi = [-h - 0.1 for h in half], [h + 0.1 for h in half]
    for voxel in (0.02, 0.01):
        vol = meshing.TsdfVolume(lo, hi, voxel, device=dev)
        for d, c, p in frames:
            vol.integrate(d, c, cam, p)
        v, f, c = vol.extract_mesh()
        del vol
        torch.cuda.empty_cache()
        full = evaluation.MeshRenderer(v, f, cam, colors=c)
        res[f"room_voxel_{voxel:g}"] = color_leg(f"room_voxel_{voxel:g}", full, cam, frames, reps, blocks, ("vertex",), parent)
        F0 = int(f.shape[0])
        del full
        v, f, c, _ = mesh_ops.decimate(v, f, c, int(0.10 * F0))
        key = f"room_voxel_{voxel:g}_decimated_10"
        try:
            image, uv, stats = meshing.texture_mesh(v, f, c, cam, [(col, p) for _, col, p in frames], texel=voxel / 2, tolerance=voxel)
        except ValueError as e:                                                # the atlas would pass 16384: say so, go on
            res[key] = {"F": int(f.shape[0]), "texel": voxel / 2, "refused": str(e)}
            continue
        small = evaluation.MeshRenderer(v, f, cam, colors=c, uv=uv, texture=image)
        res[key] = color_leg(key, small, cam, frames, reps, blocks, ("vertex", "texture"), parent)
        res[key]["texel"] = voxel / 2
        del small, image, uv, v, f, c
        torch.cuda.empty_cache()
    _finish(res, out_path)


def main():
    argv = [a for a in sys.argv[1:] if a != "--color" and not a.startswith("--parent-lib=")]
    if "--color" in sys.argv[1:]:
        parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--parent-lib=")), None)
        return color_main(argv[0] if argv else None, int(argv[1]) if len(argv) > 1 else 10, int(argv[2]) if len(argv) > 2 else 5, parent)
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
