"""Times the mesher (rtg_slam_amd.meshing) on the device and prints one JSON line (also written to OUT when given):
  * rtgs_tsdf_integrate per frame at 1200 x 680 (the Replica camera in the box room, poses of synth.room_tour) into the
    room-sized volume (the room padded by 10 cm) at 2 cm and at 1 cm voxels, in the block-skipping and in the dense form, on the
    same frames and the same (already fused) planes; the voxels a frame updates are counted from the weight plane, the bytes
    moved are 40 B per updated voxel (20 B read, 20 B written) plus the frame (16 B per pixel, read at least once);
  * the streaming yardstick of the dense form: a volume that lies wholly inside the frustum and in front of the surface, so
    that every voxel is updated and the launch moves exactly 40 B per voxel;
  * extract_mesh of the fused room at both voxel sizes (count + scan + emit + weld), with V and F;
  * the box-room end-to-end case of tests/test_mesh_gpu.py (sensor depth, 20 frames, 2 cm): vertex-to-wall statistics;
  * the sparse leg (key "sparse"; alone with --sparse-only): SparseTsdfVolume against TsdfVolume's block form on the same
    room and frames at 2 cm and 1 cm - per-frame integrate time (mark + scan + the host's read of the new-brick count +
    allocate + integrate, on volumes that already hold the frames) in alternating blocks of the same run, extraction time,
    pool bytes against dense bytes, and that the two meshes agree in V and F - and one sparse-only run at 4 mm, where the dense
    planes (1300 x 800 x 1550 x 20 B) are over TsdfVolume's cap;
  * the clean-up leg (key "cleanup"; alone with --cleanup): rtg_slam_amd.mesh_ops on the fused room's mesh at 2 cm and 1 cm -
    vertex_normals, component_labels, remove_small_components (100 faces), compact and simplify_clusters (2.5 voxels), each
    whole call (its torch sorts and scans and the host's reads of the counts included) in blocks of its own, with the counts
    before and after and the removal's statistics;
  * the decimation leg (key "decimate"; alone with --decimate): mesh_ops.decimate of the same two meshes to 25 % and to 10 % of
    their faces - whole calls (every round's kernels, torch sorts and host reads), one call per block after one warm-up call,
    rounds, collapses per round and milliseconds per round; for quality, the mean and the maximum distance from 1 M points
    sampled on the decimated mesh to the ORIGINAL mesh's vertices (evaluation's nearest-neighbour kernels; the original's
    vertices lie at most a cell's diagonal apart, so this is the deviation from the original surface up to that), and beside
    it the same figures, and the time, for simplify_clusters at the cell (a multiple of a quarter voxel) whose face count
    comes nearest;
  * the distance leg (key "distance"; alone with --distance): mesh_ops.MeshDistance on the same two meshes - the build (count, scan,
    fill, blocks and its one host read, by the events of MeshDistance.report()) and the query of 1 M points (a) sampled on the mesh
    itself, (b) sampled on its decimation to 25 %, (c) uniform in the padded box - the far case -, each at 1, 2 and 4 mean
    edge lengths as the cell, with and without the query sort, and beside them knn_query_built of the same points against the
    mesh's vertices, the thing it replaces; then the quality columns of the decimation table with this ruler, two-sided: the
    result's samples to the original SURFACE and the original's samples to the result's surface, mean and maximum, for
    decimate to 25 % and 10 % and the simplify_clusters rows beside them.  A query that takes long is timed with fewer calls
    per block (reps_per_block says how many);
  * the registration leg (key "register"; alone with --register): mesh_ops.register_to_mesh of 1 M samples of the same two
    meshes, moved by a known 1 degree rotation and 2 cm translation, back onto them - the whole call, its queries and its
    accumulations per iteration, the iteration count, what is left of the known displacement, and rtgs_mesh_register_accumulate
    alone;
  * the bounded leg (key "distance_bounded"; alone with --distance-bounded): MeshDistance.query(max_distance=D) against the
    unbounded query on the same two meshes at the default cell, sorted, in alternating blocks - 1 M points (a) sampled on the
    mesh itself, (b) uniform in the padded box, each unbounded and at D = 0.10 and 0.03 with the share of the rows within the
    bound - and (c) register_to_mesh of --register's case with 10 % of the samples replaced by points uniform in the box,
    bounded_query False and True: the whole call and the query per iteration, with the check that both return the same T;
  * the texture leg (key "texture"; alone with --texture): meshing.TextureBaker on the same two meshes, each decimated to 10 %
    of its faces, at a texel of half the voxel - the layout (levels, torch's sort and scan, face_layout, texel_face: the
    baker's own events, one construction per block after a warm-up), rtgs_mesh_texture_bake_view per view at 1200 x 680 with
    the depth maps rendered beforehand, the mesh render of the same views beside it, the finish, the atlas size, fill and seen
    share after the frames, and the bytes a view moves (4 B per atlas texel for the face map, 32 B per contributing texel)
    against the time.
Timing: device events around `reps` launches, after warm-up, in `blocks` blocks; the median block and the spread of the
blocks are reported.
python tools/mesh_check.py [--sparse-only | --cleanup | --decimate | --distance | --register | --distance-bounded | --texture] [OUT] [reps = 10] [blocks = 5]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtg_slam_amd import mesh_ops, meshing, synth   # noqa: E402


def blocks_ms(fn, reps, blocks, warmup=3):
    """fn(i) launches the i-th call; -> per-call milliseconds of every block."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(reps):
            fn(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return {"median_ms": round(float(np.median(out)), 4), "min_ms": round(float(np.min(out)), 4),
            "max_ms": round(float(np.max(out)), 4), "reps_per_block": reps, "blocks": blocks}


def _summary(ms, reps):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "reps_per_block": reps, "blocks": len(ms)}


def alternating_blocks_ms(fns, reps, blocks, warmup=3):
    """blocks_ms for several forms in one run: block k of every form before block k + 1 of any."""
    for fn in fns.values():
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(reps):
                fn(i)
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / reps)
    return {name: _summary(ms, reps) for name, ms in out.items()}


def _timed_extract(vol, runs=3):
    ext = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v, f, c = vol.extract_mesh()
        torch.cuda.synchronize()
        ext.append(time.perf_counter() - t0)
    return {"median_s": round(float(np.median(ext)), 4), "min_s": round(min(ext), 4), "max_s": round(max(ext), 4), "runs": runs,
            "V": int(v.shape[0]), "F": int(f.shape[0])}


def _fuse_all(vol, frames, cam):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for d, c, p in frames:
        vol.integrate(d, c, cam, p)
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / len(frames), 4)


def sparse_leg(dev, cam, frames, lo, hi, reps, blocks):
    res = {"timing": "device events around reps integrate calls, sparse and dense (block form) blocks alternating; the sparse "
                     "call holds one host synchronisation (the new-brick count)"}
    for voxel in (0.02, 0.01):
        sparse = meshing.SparseTsdfVolume(lo, hi, voxel, device=dev)
        dense = meshing.TsdfVolume(lo, hi, voxel, device=dev)
        entry = {"dims": list(sparse.dims), "first_pass_wall_ms_per_frame": {"sparse": _fuse_all(sparse, frames, cam),
                                                                             "dense": _fuse_all(dense, frames, cam)}}
        call = lambda vol: (lambda i: vol.integrate(*frames[i % len(frames)][:2], cam, frames[i % len(frames)][2]))
        entry["integrate"] = alternating_blocks_ms({"sparse": call(sparse), "dense_block": call(dense)}, reps, blocks)
        entry["sparse_over_dense_time_ratio"] = round(entry["integrate"]["sparse"]["median_ms"]
                                                      / entry["integrate"]["dense_block"]["median_ms"], 3)
        n_table = int(np.prod(sparse.brick_dims))
        entry.update({"bricks": sparse.n_bricks, "brick_share": round(sparse.n_bricks / n_table, 4),
                      "brick_bytes": sparse.n_bricks * meshing.BRICK_BYTES, "pool_bytes": sparse.pool_bytes,
                      "table_bytes": 4 * n_table, "dense_bytes": sparse.dense_bytes,
                      "pool_over_dense_bytes": round(sparse.pool_bytes / sparse.dense_bytes, 4),
                      "updated_share_dense": round(float((dense.weight > 0).float().mean()), 4)})
        entry["extract"] = {"sparse": _timed_extract(sparse), "dense": _timed_extract(dense)}
        entry["same_V_and_F"] = all(entry["extract"]["sparse"][k] == entry["extract"]["dense"][k] for k in ("V", "F"))
        res[f"room_voxel_{voxel:g}"] = entry
        del sparse, dense
        torch.cuda.empty_cache()
    voxel = 0.004
    refused = None
    try:
        meshing.TsdfVolume(lo, hi, voxel, device=dev)
    except ValueError as e:
        refused = str(e)
    sparse = meshing.SparseTsdfVolume(lo, hi, voxel, device=dev)
    entry = {"dims": list(sparse.dims), "dense_refuses": refused, "first_pass_wall_ms_per_frame": _fuse_all(sparse, frames, cam)}
    entry["integrate"] = blocks_ms(lambda i: sparse.integrate(*frames[i % len(frames)][:2], cam, frames[i % len(frames)][2]), reps,
                                   blocks)
    n_table = int(np.prod(sparse.brick_dims))
    entry.update({"bricks": sparse.n_bricks, "brick_share": round(sparse.n_bricks / n_table, 4),
                  "brick_bytes": sparse.n_bricks * meshing.BRICK_BYTES, "pool_bytes": sparse.pool_bytes, "table_bytes": 4 * n_table,
                  "dense_bytes": sparse.dense_bytes, "pool_over_dense_bytes": round(sparse.pool_bytes / sparse.dense_bytes, 4)})
    entry["extract"] = _timed_extract(sparse)
    res[f"room_voxel_{voxel:g}_sparse_only"] = entry
    return res


def cleanup_leg(dev, cam, frames, lo, hi, reps, blocks):
    res = {"timing": "device events around reps whole calls of one operation (kernels, torch sorts / scans, and the host reads "
                     "of counts that size the outputs), blocks after a warm-up of 3 calls",
           "min_faces": 100, "simplify_cell_voxels": 2.5}
    for voxel in (0.02, 0.01):
        vol = meshing.TsdfVolume(lo, hi, voxel, device=dev)
        _fuse_all(vol, frames, cam)
        entry = {"dims": list(vol.dims), "extract": _timed_extract(vol)}
        v, f, c = vol.extract_mesh()
        origin = vol.lo
        del vol
        torch.cuda.empty_cache()
        cell = 2.5 * voxel
        entry["vertex_normals"] = blocks_ms(lambda i: mesh_ops.vertex_normals(v, f), reps, blocks)
        entry["component_labels"] = blocks_ms(lambda i: mesh_ops.component_labels(f, v.shape[0]), reps, blocks)
        entry["remove_small_components"] = blocks_ms(lambda i: mesh_ops.remove_small_components(v, f, c, 100), reps, blocks)
        entry["compact"] = blocks_ms(lambda i: mesh_ops.compact(v, f, c), reps, blocks)
        entry["simplify_clusters"] = blocks_ms(lambda i: mesh_ops.simplify_clusters(v, f, c, cell, origin), reps, blocks)
        rv, rf, rc, stats = mesh_ops.remove_small_components(v, f, c, 100)
        sv, sf, sc = mesh_ops.simplify_clusters(rv, rf, rc, cell, origin)
        n = mesh_ops.vertex_normals(sv, sf)
        entry.update({"V": int(v.shape[0]), "F": int(f.shape[0]), "removal": stats, "V_after_removal": int(rv.shape[0]),
                      "F_after_removal": int(rf.shape[0]), "simplify_cell": cell, "V_after_simplify": int(sv.shape[0]),
                      "F_after_simplify": int(sf.shape[0]), "zero_normals_after_simplify": int((n.abs().sum(1) == 0).sum())})
        res[f"room_voxel_{voxel:g}"] = entry
        del v, f, c, rv, rf, rc, sv, sf, sc, n
        torch.cuda.empty_cache()
    return res


def _deviation(v, f, original_index, n_original, seed=0):
    """1 M points sampled on the mesh (v, f) -> their distance to the nearest vertex of the original mesh."""
    from rtg_slam_amd import evaluation as ev, slam_ops as so
    pts = ev.sample_mesh_points(v, f, 1_000_000, seed, v.device).contiguous()
    d2, _ = so.knn_query_built(original_index, n_original, pts)
    d = d2[:, 0].double().sqrt()
    return {"mean_m": float(d.mean()), "max_m": float(d.max()), "p99_m": float(torch.quantile(d[::10], 0.99))}


def decimate_leg(dev, cam, frames, lo, hi, blocks):
    from rtg_slam_amd import slam_ops as so
    res = {"timing": "device events around ONE whole mesh_ops.decimate call per block (every round's kernels, torch sorts and "
                     "scans and host reads of counts), blocks after one warm-up call",
           "quality": "distance from 1 M points sampled on the result to the nearest vertex of the original mesh"}
    for voxel in (0.02, 0.01):
        vol = meshing.TsdfVolume(lo, hi, voxel, device=dev)
        _fuse_all(vol, frames, cam)
        entry = {"dims": list(vol.dims), "extract": _timed_extract(vol)}
        v, f, c = vol.extract_mesh()
        origin = vol.lo
        del vol
        torch.cuda.empty_cache()
        V, F = int(v.shape[0]), int(f.shape[0])
        entry.update({"V": V, "F": F})
        index = so.knn_build_ref(v.contiguous())
        entry["original_sampled"] = _deviation(v, f, index, V)
        cells = {}
        for i in range(36):
            cell = voxel * (1.25 + 0.25 * i)
            cells[cell] = int(mesh_ops.simplify_clusters(v, f, c, cell, origin)[1].shape[0])
        for share in (0.25, 0.10):
            target = int(share * F)
            ov, of, oc, stats = mesh_ops.decimate(v, f, c, target)
            e = {"target_faces": target, "V_after": int(ov.shape[0]), "F_after": int(of.shape[0]), **stats,
                 "collapses_per_round": round(stats["collapses"] / max(stats["rounds"], 1), 1)}
            e["call"] = blocks_ms(lambda i: mesh_ops.decimate(v, f, c, target), 1, blocks, warmup=1)
            e["ms_per_round"] = round(e["call"]["median_ms"] / max(stats["rounds"], 1), 4)
            e["deviation"] = _deviation(ov, of, index, V)
            n = mesh_ops.vertex_normals(ov, of)
            e["zero_normals"] = int((n.abs().sum(1) == 0).sum())
            cell = min(cells, key=lambda k: abs(cells[k] - int(of.shape[0])))
            sv, sf, sc = mesh_ops.simplify_clusters(v, f, c, cell, origin)
            n = mesh_ops.vertex_normals(sv, sf)
            e["simplify_clusters"] = {"cell": cell, "cell_voxels": round(cell / voxel, 2), "V_after": int(sv.shape[0]),
                                      "F_after": int(sf.shape[0]), "deviation": _deviation(sv, sf, index, V),
                                      "zero_normals": int((n.abs().sum(1) == 0).sum()),
                                      "call": blocks_ms(lambda i: mesh_ops.simplify_clusters(v, f, c, cell, origin), 10, blocks)}
            entry[f"to_{int(100 * share)}_percent"] = e
            del ov, of, oc, sv, sf, sc, n
        res[f"room_voxel_{voxel:g}"] = entry
        del v, f, c, index
        torch.cuda.empty_cache()
    return res


def _adaptive_ms(fn, reps, blocks):
    """blocks_ms, with fewer calls per block when one call is slow: about half a second of calls per block."""
    fn(0)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(0)
    b.record()
    b.synchronize()
    first = a.elapsed_time(b)
    reps = max(1, min(reps, int(500.0 / max(first, 1e-3))))
    return blocks_ms(fn, reps, blocks if first < 1000.0 else 2, warmup=0)


def _surface_deviation(md, pts):
    d = md.query(pts)[0].double().sqrt()
    return {"mean_m": float(d.mean()), "max_m": float(d.max())}


def distance_leg(dev, cam, frames, lo, hi, reps, blocks):
    from rtg_slam_amd import evaluation as ev, slam_ops as so
    res = {"timing": "device events; the build is MeshDistance's own pair of events around count, scan, fill and blocks (one host "
                     "read inside), the median of `blocks` builds after one; a query is one whole md.query call of 1 M points "
                     "(with sort: the key kernel and torch's sort included), reps calls per block, fewer when a call is slow",
           "points": {"self": "1 M samples of the mesh itself", "decimated": "1 M samples of its decimation to 25 %",
                      "far": "1 M points uniform in the padded box"}}
    n = 1_000_000
    for voxel in (0.02, 0.01):
        vol = meshing.TsdfVolume(lo, hi, voxel, device=dev)
        _fuse_all(vol, frames, cam)
        v, f, c = vol.extract_mesh()
        origin = vol.lo
        del vol
        torch.cuda.empty_cache()
        V, F = int(v.shape[0]), int(f.shape[0])
        tri = v[f.reshape(-1).long()].reshape(F, 3, 3)
        mean_edge = float((tri - tri.roll(-1, 1)).double().norm(dim=2).mean())
        del tri
        entry = {"V": V, "F": F, "mean_edge_m": mean_edge}
        dv, df, dc, _ = mesh_ops.decimate(v, f, c, int(0.25 * F))
        gen = torch.Generator().manual_seed(0)
        box_lo, box_hi = torch.tensor(lo), torch.tensor(hi)
        sets = {"self": ev.sample_mesh_points(v, f, n, 0, dev).contiguous(), "decimated": ev.sample_mesh_points(dv, df, n, 0, dev).contiguous(),
                "far": (box_lo + (box_hi - box_lo) * torch.rand(n, 3, generator=gen)).to(dev).contiguous()}
        index = so.knn_build_ref(v.contiguous())
        entry["knn_query_built_vertices"] = {k: _adaptive_ms(lambda i, p=p: so.knn_query_built(index, V, p), reps, blocks) for k, p in sets.items()}
        for mult in (1, 2, 4):
            e = {"cell": mult * mean_edge}
            try:
                builds = [mesh_ops.MeshDistance(v, f, cell=mult * mean_edge).report()["build_s"] for _ in range(blocks + 1)][1:]
            except ValueError as err:
                e["refused"] = str(err)
                entry[f"cell_{mult}_edges"] = e
                continue
            print(f"distance: voxel {voxel:g}, cell {mult} edges: built", file=sys.stderr, flush=True)
            e["build"] = {"median_ms": round(1e3 * float(np.median(builds)), 4), "min_ms": round(1e3 * min(builds), 4),
                          "max_ms": round(1e3 * max(builds), 4), "blocks": blocks}
            for sort in (False, True):
                md = mesh_ops.MeshDistance(v, f, cell=mult * mean_edge, sort=sort)
                if not sort:
                    e.update({k: md.report()[k] for k in ("dims", "cells", "entries", "bytes", "large_faces")})
                e["query_sorted" if sort else "query"] = {k: _adaptive_ms(lambda i, p=p: md.query(p), reps, blocks) for k, p in sets.items()}
                del md
            entry[f"cell_{mult}_edges"] = e
        print(f"distance: voxel {voxel:g}: queries timed", file=sys.stderr, flush=True)
        # the decimation table's quality columns with this ruler, two-sided
        md = mesh_ops.MeshDistance(v, f)
        entry["default_cell"] = md.report()["cell"]
        entry["original_to_itself"] = _surface_deviation(md, sets["self"])
        cells = {}
        for i in range(36):
            cell = voxel * (1.25 + 0.25 * i)
            cells[cell] = int(mesh_ops.simplify_clusters(v, f, c, cell, origin)[1].shape[0])
        for share in (0.25, 0.10):
            ov, of, oc, _ = mesh_ops.decimate(v, f, c, int(share * F))
            cell = min(cells, key=lambda k: abs(cells[k] - int(of.shape[0])))
            sv, sf, sc = mesh_ops.simplify_clusters(v, f, c, cell, origin)
            row = {}
            for name, (rv, rf) in (("decimate", (ov, of)), ("simplify_clusters", (sv, sf))):
                row[name] = {"F_after": int(rf.shape[0]),
                             "result_to_original": _surface_deviation(md, ev.sample_mesh_points(rv, rf, n, 0, dev).contiguous()),
                             "original_to_result": _surface_deviation(mesh_ops.MeshDistance(rv, rf), sets["self"])}
            row["simplify_clusters"]["cell"] = cell
            entry[f"to_{int(100 * share)}_percent"] = row
            del ov, of, oc, sv, sf, sc
        res[f"room_voxel_{voxel:g}"] = entry
        del v, f, c, dv, df, dc, md, index, sets
        torch.cuda.empty_cache()
    return res


def register_leg(dev, cam, frames, lo, hi, reps, blocks):
    from rtg_slam_amd import evaluation as ev
    res = {"timing": "one whole mesh_ops.register_to_mesh call of 1 M points per block after one warm-up call: device events around "
                     "the call (every iteration's transform, query, accumulation, host read and solve), and the report's own "
                     "events around the queries and the accumulations, divided by the accumulations; accumulate_alone: "
                     "register_accumulate of the same points on a query's result, reps calls per block",
           "known": "the samples are moved by the inverse of a 1 degree rotation about (0.4, -0.7, 0.59) and a 2 cm translation"}
    n = 1_000_000
    axis = np.array([0.4, -0.7, 0.59]) / np.linalg.norm([0.4, -0.7, 0.59])
    known = np.eye(4)
    known[:3, :3] = mesh_ops._rodrigues(axis * np.deg2rad(1.0))
    known[:3, 3] = 0.02 * np.array([0.6, -0.5, 0.62]) / np.linalg.norm([0.6, -0.5, 0.62])
    for voxel in (0.02, 0.01):
        vol = meshing.TsdfVolume(lo, hi, voxel, device=dev)
        _fuse_all(vol, frames, cam)
        v, f, _ = vol.extract_mesh()
        del vol
        torch.cuda.empty_cache()
        md = mesh_ops.MeshDistance(v, f)
        true = ev.sample_mesh_points(v, f, n, 0, dev).double()
        inv = torch.from_numpy(np.linalg.inv(known)).to(dev)
        src = (true @ inv[:3, :3].T + inv[:3, 3]).float().contiguous()
        entry = {"V": int(v.shape[0]), "F": int(f.shape[0]), "points": n, "cell": md.report()["cell"]}
        calls = []
        for k in range(blocks + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            T, rep = mesh_ops.register_to_mesh(src, md)
            b.record()
            b.synchronize()
            passes = len(rep["inliers"])
            calls.append({"call_ms": a.elapsed_time(b), "query_ms_per_pass": 1e3 * rep["query_s"] / passes,
                          "accumulate_ms_per_pass": 1e3 * rep["accumulate_s"] / passes})
        calls = calls[1:]
        for key in ("call_ms", "query_ms_per_pass", "accumulate_ms_per_pass"):
            entry[key] = _summary([c[key] for c in calls], 1)
        Tt = torch.from_numpy(T).to(dev)
        entry["residual_displacement_m"] = float(((src.double() @ Tt[:3, :3].T + Tt[:3, 3]) - true).norm(dim=1).max())
        entry["report"] = {k: rep[k] for k in ("iterations", "converged", "reason", "inliers", "inlier_share", "rank", "rotation_deg",
                                               "translation_m", "rms_plane_before", "rms_plane_after", "rms_distance_before",
                                               "rms_distance_after")}
        d2, face = md.query(src)
        center = (md.box[0] + md.box[1]) * 0.5
        entry["accumulate_alone"] = blocks_ms(lambda i: mesh_ops.register_accumulate(src, face, d2, md, center, 0.01), reps, blocks)
        entry["accumulate_alone"]["bytes_per_point"] = "12 point + 4 face + 4 d2 read, 12 face indices and 36 corner gathered"
        res[f"room_voxel_{voxel:g}"] = entry
        print(f"register: voxel {voxel:g} done", file=sys.stderr, flush=True)
        del v, f, md, src, true, d2, face
        torch.cuda.empty_cache()
    return res


def _adaptive_alternating_ms(fns, reps, blocks):
    """alternating_blocks_ms with _adaptive_ms's calls per block: every form gets its own count from one timed call after a
    warm-up call, and all forms run 2 blocks when one call of any takes more than a second."""
    counts, slow = {}, False
    for name, fn in fns.items():
        fn(0)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(0)
        b.record()
        b.synchronize()
        first = a.elapsed_time(b)
        counts[name] = max(1, min(reps, int(500.0 / max(first, 1e-3))))
        slow = slow or first >= 1000.0
    out = {name: [] for name in fns}
    for _ in range(2 if slow else blocks):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(counts[name]):
                fn(i)
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / counts[name])
    return {name: _summary(ms, counts[name]) for name, ms in out.items()}


BOUNDS = (0.10, 0.03)


def bounded_leg(dev, cam, frames, lo, hi, reps, blocks):
    from rtg_slam_amd import evaluation as ev
    res = {"timing": "device events around whole md.query calls of 1 M points (the key kernel and torch's sort included), default "
                     "cell, sort on; the unbounded query and the bounded one at every D in alternating blocks, the calls per block "
                     "set per form from one timed call (2 blocks when a call takes more than a second); register: one whole "
                     "register_to_mesh call per block after a warm-up call, bounded_query False and True alternating",
           "points": {"self": "1 M samples of the mesh itself", "far": "1 M points uniform in the padded box",
                      "register": "--register's 1 M moved samples, every 10th replaced by a point uniform in the padded box"},
           "max_distance_m": list(BOUNDS)}
    n = 1_000_000
    axis = np.array([0.4, -0.7, 0.59]) / np.linalg.norm([0.4, -0.7, 0.59])
    known = np.eye(4)
    known[:3, :3] = mesh_ops._rodrigues(axis * np.deg2rad(1.0))
    known[:3, 3] = 0.02 * np.array([0.6, -0.5, 0.62]) / np.linalg.norm([0.6, -0.5, 0.62])
    for voxel in (0.02, 0.01):
        vol = meshing.TsdfVolume(lo, hi, voxel, device=dev)
        _fuse_all(vol, frames, cam)
        v, f, _ = vol.extract_mesh()
        del vol
        torch.cuda.empty_cache()
        md = mesh_ops.MeshDistance(v, f, sort=True)
        entry = {"V": int(v.shape[0]), "F": int(f.shape[0]), "cell": md.report()["cell"]}
        gen = torch.Generator().manual_seed(0)
        box_lo, box_hi = torch.tensor(lo), torch.tensor(hi)
        uniform = (box_lo + (box_hi - box_lo) * torch.rand(n, 3, generator=gen)).to(dev).contiguous()
        own = ev.sample_mesh_points(v, f, n, 0, dev).contiguous()
        for name, p in (("self", own), ("far", uniform)):
            fns = {"unbounded": lambda i, p=p: md.query(p)}
            for D in BOUNDS:
                fns[f"bounded_{D:g}"] = lambda i, p=p, D=D: md.query(p, max_distance=D)
            row = _adaptive_alternating_ms(fns, reps, blocks)
            d2u, fu = md.query(p)
            for D in BOUNDS:
                d2b, fb = md.query(p, max_distance=D)
                kept = fb >= 0
                row[f"bounded_{D:g}"]["share_within"] = float(kept.float().mean())
                row[f"bounded_{D:g}"]["rows_within_equal_unbounded"] = bool(torch.equal(d2b[kept], d2u[kept]) and torch.equal(fb[kept], fu[kept])
                                                                            and bool((d2u[~kept] > np.float32(D) * np.float32(D)).all()))
            entry[name] = row
            print(f"distance-bounded: voxel {voxel:g}, {name}: timed", file=sys.stderr, flush=True)
        inv = torch.from_numpy(np.linalg.inv(known)).to(dev)
        src = (own.double() @ inv[:3, :3].T + inv[:3, 3]).float().contiguous()
        src[::10] = uniform[::10]
        calls = {False: [], True: []}
        last = {}
        for k in range(blocks + 1):
            for bounded in (False, True):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                T, rep = mesh_ops.register_to_mesh(src, md, bounded_query=bounded)
                b.record()
                b.synchronize()
                passes = len(rep["inliers"])
                calls[bounded].append({"call_ms": a.elapsed_time(b), "query_ms_per_pass": 1e3 * rep["query_s"] / passes,
                                       "accumulate_ms_per_pass": 1e3 * rep["accumulate_s"] / passes})
                last[bounded] = (T, rep)
        reg = {"points": n, "max_distance": 0.10}
        for bounded in (False, True):
            reg["bounded_query" if bounded else "unbounded_query"] = {
                key: _summary([c[key] for c in calls[bounded][1:]], 1) for key in ("call_ms", "query_ms_per_pass", "accumulate_ms_per_pass")}
        reg["same_T_and_inliers"] = bool(np.array_equal(last[False][0], last[True][0]) and last[False][1]["inliers"] == last[True][1]["inliers"])
        reg["report"] = {k: last[True][1][k] for k in ("iterations", "converged", "reason", "inliers", "inlier_share")}
        entry["register"] = reg
        res[f"room_voxel_{voxel:g}"] = entry
        print(f"distance-bounded: voxel {voxel:g} done", file=sys.stderr, flush=True)
        del v, f, md, own, uniform, src
        torch.cuda.empty_cache()
    return res


def texture_leg(dev, cam, frames, lo, hi, reps, blocks):
    res = {"timing": "device events; layout: the baker's own events around levels + sort + scan + face_layout + texel_face, one "
                     "construction per block after a warm-up; bake and render: `reps` launches per block over the frames in turn",
           "bytes": "per view: 4 B per atlas texel (texel_face) + 32 B per contributing texel (16 B of acc read and written)"}
    for voxel in (0.02, 0.01):
        vol = meshing.TsdfVolume(lo, hi, voxel, device=dev)
        _fuse_all(vol, frames, cam)
        v, f, c = vol.extract_mesh()
        del vol
        torch.cuda.empty_cache()
        F0 = int(f.shape[0])
        v, f, c, dstats = mesh_ops.decimate(v, f, c, int(0.10 * F0))
        texel = voxel / 2
        make = lambda: meshing.TextureBaker(v, f, cam, texel=texel, tolerance=voxel)
        try:
            layout = [make().layout_s * 1e3 for _ in range(blocks + 1)][1:]
        except ValueError as e:                                                # the atlas would pass 16384: say so, go on
            res[f"room_voxel_{voxel:g}"] = {"F": int(f.shape[0]), "texel": texel, "refused": str(e)}
            continue
        baker = make()
        Wt, Ht = baker.size
        entry = {"F_extracted": F0, "V": int(v.shape[0]), "F": int(f.shape[0]), "decimate_target_reached": dstats["target_reached"],
                 "texel": texel, "size": [Wt, Ht], "atlas_texels": Wt * Ht, "texels_assigned": baker.T, "fill": round(baker.T / (Wt * Ht), 4),
                 "faces_capped": int(baker.capped.sum()),
                 "levels": torch.bincount(baker.levels.to(torch.int64), minlength=7)[1:7].tolist(), "layout": _summary(layout, 1)}
        depths = [baker.renderer.render(p)[0] for _, _, p in frames]
        contributing = []
        for (_, col, p), d in zip(frames, depths):
            before = baker.acc[..., 3].clone()
            baker.bake(col, d, p)
            contributing.append(int((baker.acc[..., 3] != before).sum()))
            del before
        image, flags = baker.finish(c)
        seen = int((flags == 2).sum())
        moved = 4.0 * Wt * Ht + 32.0 * float(np.mean(contributing))
        entry.update({"views": len(frames), "texels_seen": seen, "seen_share": round(seen / max(baker.T, 1), 4),
                      "contributing_texels_per_view_mean": int(np.mean(contributing)), "bytes_moved_per_view_mean": int(moved)})
        n = len(frames)
        timed = alternating_blocks_ms({"bake_view": lambda i: baker.bake(frames[i % n][1], depths[i % n], frames[i % n][2]),
                                       "mesh_render": lambda i: baker.renderer.render(frames[i % n][2])}, reps, blocks)
        timed["bake_view"]["TB_per_s_of_moved_bytes_at_median"] = round(moved / (timed["bake_view"]["median_ms"] * 1e-3) / 1e12, 3)
        entry.update(timed)
        entry["finish"] = blocks_ms(lambda i: baker.finish(c), reps, blocks)
        res[f"room_voxel_{voxel:g}"] = entry
        del baker, depths, image, flags, v, f, c
        torch.cuda.empty_cache()
    return res


def main():
    argv = [a for a in sys.argv[1:] if a not in ("--sparse-only", "--cleanup", "--decimate", "--distance", "--register", "--distance-bounded",
                                                 "--texture")]
    sparse_only = "--sparse-only" in sys.argv[1:]
    cleanup_only = "--cleanup" in sys.argv[1:]
    out_path = argv[0] if len(argv) > 0 else None
    reps = int(argv[1]) if len(argv) > 1 else 10
    blocks = int(argv[2]) if len(argv) > 2 else 5
    dev = torch.device("cuda", 0)
    cam = synth.REPLICA
    res = {"device": torch.cuda.get_device_name(dev), "camera": [cam.W, cam.H], "bytes_per_updated_voxel": 40}
    poses = synth.room_tour(reps * 40, seed=3)[::40]
    frames = []
    for p in poses:
        d = synth.box_room_depth(cam, p, device=dev)
        frames.append((d.reshape(cam.H, cam.W).contiguous(), synth.box_room_color(cam, p, d), p.numpy()))
    frame_bytes = cam.H * cam.W * 16
    half = (2.5, 1.5, 3.0)
    lo, hi = [-h - 0.1 for h in half], [h + 0.1 for h in half]
    if "--distance" in sys.argv[1:]:
        res["distance"] = distance_leg(dev, cam, frames, lo, hi, reps, blocks)
        return _finish(res, out_path)
    if "--distance-bounded" in sys.argv[1:]:
        res["distance_bounded"] = bounded_leg(dev, cam, frames, lo, hi, reps, blocks)
        return _finish(res, out_path)
    if "--register" in sys.argv[1:]:
        res["register"] = register_leg(dev, cam, frames, lo, hi, reps, blocks)
        return _finish(res, out_path)
    if "--texture" in sys.argv[1:]:
        res["texture"] = texture_leg(dev, cam, frames, lo, hi, reps, blocks)
        return _finish(res, out_path)
    if "--decimate" in sys.argv[1:]:
        res["decimate"] = decimate_leg(dev, cam, frames, lo, hi, blocks)
        return _finish(res, out_path)
    if cleanup_only:
        res["cleanup"] = cleanup_leg(dev, cam, frames, lo, hi, reps, blocks)
        return _finish(res, out_path)
    if sparse_only:
        res["sparse"] = sparse_leg(dev, cam, frames, lo, hi, reps, blocks)
        return _finish(res, out_path)
    for voxel in (0.02, 0.01):
        vol = meshing.TsdfVolume(lo, hi, voxel, device=dev)
        n = vol.dims[0] * vol.dims[1] * vol.dims[2]
        updated = []
        for d, c, p in frames:
            before = vol.weight.clone()
            vol.integrate(d, c, cam, p)
            updated.append(int((vol.weight != before).sum()))
            del before
        entry = {"dims": list(vol.dims), "voxels": n, "plane_bytes": n * 20,
                 "updated_voxels_per_frame_mean": int(np.mean(updated)), "updated_share_mean": round(float(np.mean(updated)) / n, 4)}
        moved = float(np.mean(updated)) * 40 + frame_bytes
        entry["bytes_moved_per_frame_mean"] = int(moved)
        call = lambda i: vol.integrate(*frames[i % len(frames)][:2], cam, frames[i % len(frames)][2])
        for form in ("block", "dense"):
            meshing.set_dense_form(form == "dense")
            try:
                t = blocks_ms(call, reps, blocks)
            finally:
                meshing.set_dense_form(False)
            t["TB_per_s_of_moved_bytes_at_median"] = round(moved / (t["median_ms"] * 1e-3) / 1e12, 3)
            entry[form] = t
        entry["block_over_dense_time_ratio"] = round(entry["block"]["median_ms"] / entry["dense"]["median_ms"], 3)
        torch.cuda.synchronize()
        ext = []
        for _ in range(3):
            t0 = time.perf_counter()
            v, f, c = vol.extract_mesh()
            torch.cuda.synchronize()
            ext.append(time.perf_counter() - t0)
        entry["extract"] = {"median_s": round(float(np.median(ext)), 4), "min_s": round(min(ext), 4), "max_s": round(max(ext), 4),
                            "runs": 3, "V": int(v.shape[0]), "F": int(f.shape[0]),
                            "bytes_read_lower_bound": n * 8 + n * 4 + int(f.shape[0]) * 3 * 32,
                            "includes": "count, cumsum, emit, unique / inverse weld, gathers; wall clock with a final synchronise"}
        res[f"room_voxel_{voxel:g}"] = entry
        del vol, v, f, c
        torch.cuda.empty_cache()

    # streaming yardstick: every voxel inside the frustum and in front of a constant 10 m depth
    voxel = 0.008
    vol = meshing.TsdfVolume((-1.9, -1.1, 2.0), (1.9, 1.1, 4.0), voxel, device=dev)
    n = vol.dims[0] * vol.dims[1] * vol.dims[2]
    depth = torch.full((cam.H, cam.W), 10.0, device=dev)
    color = frames[0][1]
    vol.integrate(depth, color, cam, np.eye(4))
    assert int((vol.weight == 1).sum()) == n, "the yardstick volume must be updated everywhere"
    entry = {"dims": list(vol.dims), "voxels": n, "bytes_moved": n * 40 + frame_bytes,
             "yardstick": "rtgs_densify_discs writes at 5.0-5.3 TB/s on this chip (profiles/r09_densify_check.json)"}
    for form in ("dense", "block"):
        meshing.set_dense_form(form == "dense")
        try:
            t = blocks_ms(lambda i: vol.integrate(depth, color, cam, np.eye(4)), reps, blocks)
        finally:
            meshing.set_dense_form(False)
        t["TB_per_s_at_median"] = round((n * 40 + frame_bytes) / (t["median_ms"] * 1e-3) / 1e12, 3)
        entry[form] = t
    res["all_voxels_updated"] = entry
    del vol

    # the end-to-end case of tests/test_mesh_gpu.py
    from tests import tsdf_reference as tr
    bcam, bframes, blo, bhi, bvoxel = tr.box_room_case()
    stream = [(d.to(dev), c.to(dev), p) for d, c, p in bframes]
    v, f, c, report = meshing.mesh_from_map(None, bcam, None, iter(stream), voxel=bvoxel, depth_source="sensor", bounds=(blo, bhi),
                                            device=dev)
    res["box_room_sensor_2cm"] = {"report": report, "vertex_to_wall_m": tr.wall_stats(v.cpu().numpy()),
                                  "numpy_reference_on_cpu": {"mean": 0.01126, "p99": 0.03607, "max": 0.03778, "covered": 0.1844}}
    res["sparse"] = sparse_leg(dev, cam, frames, lo, hi, reps, blocks)
    res["cleanup"] = cleanup_leg(dev, cam, frames, lo, hi, reps, blocks)
    _finish(res, out_path)


def _finish(res, out_path):
    line = json.dumps(res, default=float)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fo:
            json.dump(res, fo, indent=1, default=float)


if __name__ == "__main__":
    main()
