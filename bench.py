#!/usr/bin/env python
"""bench.py - the hot path of RTG-SLAM on MI355X, measured.

A "step" is one synthetic Replica-shaped SLAM frame on the headline configuration of
BASELINE.json (1.2 M Gaussians, 1200x680):
    1 ICP frame-to-model track (3 pyramid levels x 5 Gauss-Newton iterations, SLAM/icp.py)
  + 1 map-optimisation iteration (rasterizer forward, L1 colour + depth loss, rasterizer
    backward, fused Adam) over the whole Gaussian set (mapper.py:176-205).
`value` = frames / s over all ranks (weak scaling: every rank tracks and renders its own view; see
`config.parallelism` in the JSON line and DESIGN.md section 5 for what is exchanged).

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times exactly `--steps` frames (`ms_per_step`,
`value`) and prints the headline fields; `--full` adds the further timed blocks, `roofline` for the dominant kernel,
`cpu_baseline` (oracle on the host cores, bounded sample) and the other legs.  `--dump-outputs DIR` writes what the
last timed frame computed (dump_outputs).
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=1_200_000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-surface", action="store_true", help="skip the surface-shaped 1.2 M scene leg")
    ap.add_argument("--reserve-cus", type=int, default=32,
                    help="compute units the mapper's stream leaves to the tracker (rtgs_stream_create_reserving; 0 = none): "
                         "measured 0 / 16 / 24 / 32 / 40 / 64 -> 0.452 / 0.449 / 0.438 / 0.432 / 0.442 / 0.456 ms per unit")
    ap.add_argument("--mode", choices=["auto", "sparse", "sharded", "tileband"], default="auto",
                    help="multi-GPU form of the map step (ignored on one GPU): sparse = every rank renders its own view, "
                         "gradient rows that exist are all-gathered (in-band counts, no host sync), identical Adam step on "
                         "every replica [weak scaling]; sharded = dense reduce-scatter of the gradients, Adam on the rank's "
                         "row shard, all-gather of the updated rows [weak]; tileband = ONE view split into tile bands, "
                         "loss normalisers all-reduced, gradient rows summed by the sparse exchange [strong]; auto (default) = "
                         "tileband: a SLAM stream has ONE frame per step, so N GPUs can only split that frame - the weak-scaling "
                         "sparse form is reported beside it as `weak_scaling_one_view_per_rank`")
    ap.add_argument("--sequence-frames", type=int, default=2000,
                    help="frames of the `sequence` leg (BASELINE configs[2]: empty map, reference schedule and lifecycle, 1200x680; 2 000 = the "
                         "length of a Replica sequence, ~17 s on one MI355X)")
    ap.add_argument("--no-sequence", action="store_true")
    ap.add_argument("--no-config5", action="store_true", help="skip the BASELINE configs[4] block (5 M Gaussians, sharded, 10 iterations)")
    ap.add_argument("--config5-gaussians", type=int, default=5_000_000)
    ap.add_argument("--no-dropin", action="store_true", help="skip the unchanged-reference-iteration leg")
    ap.add_argument("--only", choices=["sequence", "config5", "icp_tum", "dropin"], default=None,
                    help="run ONE extra leg and print its JSON (profiling aid; not the contract line)")
    ap.add_argument("--prewarm", type=int, default=3000,
                    help="untimed frames of the real workload before the warm-up: a FIXED count (every rank issues the same "
                         "collectives), >= 1.5 s of GPU work - a fresh box needs that long to reach its steady clocks (the "
                         "driver's first block of round 3 ran 25 %% slower than its later ones after 0.1 s of pre-warm)")
    ap.add_argument("--repeats", type=int, default=5, help="with --full: timed blocks of --steps frames, each bracketed as the "
                                                           "contract says; their median is reported in `repeats` (`value` is "
                                                           "the first block)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline block, run everything else the line can report: further timed blocks (--repeats), "
                         "the unit taken apart, the scaling legs, the kernel profile / roofline, the surface, schedule, "
                         "sequence, TUM-ICP, drop-in and configs[4] legs, the CPU baseline.  Without it a run sets up, warms "
                         "up, times --steps frames and prints the headline fields only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32/64, "
                         "about 16 MB; see dump_outputs)")
    ap.add_argument("--surface-map", action="store_true", help="headline leg on the single-layer surface map instead of the "
                                                               "SURVEY 8d volume generator")
    ap.add_argument("--no-schedule", action="store_true", help="skip the reference-schedule leg (6 frames: 6 tracks + "
                                                               "Gaussian adding + 50 map iterations over a 5-frame window)")
    return ap.parse_args()


def source_hash():
    """sha256 over the kernel sources: PMC-derived numbers in profiles/ carry the hash they were measured at."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "rtg_slam_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def respawn_under_torchrun(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (one per GPU, RCCL) and relay rank 0's
    line - a bare run must never measure one rank and call it N."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.exit(subprocess.call(cmd, env=env))


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_under_torchrun(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
                         f"(python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ...)")
    rccl_ranks = 0
    if args.gpus > 1 or world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        # RTGS_DIST_BACKEND=gloo lets two ranks share one GPU (RCCL refuses that) to exercise this code path
        # on a single-GPU box; the driver's multi-GPU runs use nccl (= RCCL over xGMI), one rank per GPU.
        backend = os.environ.get("RTGS_DIST_BACKEND", "nccl")
        ndev = torch.cuda.device_count()
        torch.cuda.set_device(local_rank % ndev)
        if backend == "nccl":
            if ndev < world:
                raise SystemExit(f"bench.py: {world} ranks over RCCL need {world} GPUs, {ndev} visible "
                                 "(RTGS_DIST_BACKEND=gloo shares one GPU for a functional check only)")
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank % ndev))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        assert dist.get_world_size() == args.gpus and dist.get_backend() == backend
        rccl_ranks = world if backend == "nccl" else 0
    dev = torch.device("cuda", (local_rank % torch.cuda.device_count()) if world > 1 else 0)
    torch.cuda.set_device(dev)

    from rtg_slam_amd import _lib, synth, icp as hicp
    from rtg_slam_amd import map_optim as mo
    from rtg_slam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    lib = _lib.load()

    cam = synth.REPLICA
    N = args.gaussians
    if args.mode == "auto":
        args.mode = "tileband"
    if args.only is not None:
        return only_leg(args, rank, world, dev)
    one_stream = args.mode == "tileband" and world > 1        # every rank works on rank 0's frame
    # same map on every rank
    g = synth.surface_gaussians(N, cam, seed=7) if args.surface_map else synth.random_gaussians(N, cam, seed=2024)
    packed = mo.pack_from_activated({k: v.to(dev) for k, v in g.items()})
    # learning rates x1e-4: the targets are random images, at the reference's rates the map would
    # inflate within a few hundred steps and the workload would drift; Adam does identical work.
    opt = mo.ShardedMapOptimizer(packed, lr_col=mo.default_lr_columns() * 1e-4)

    # this rank's view: a small pose offset per rank (sliding-window views of one map)
    c2w = (synth.look_at_pose(seed=100 + rank, max_angle_deg=2.0, max_trans=0.05) if (world > 1 and not one_stream)
           else torch.eye(4, dtype=torch.float64))
    view = torch.linalg.inv(c2w).float().t().contiguous().to(dev)
    campos = c2w[:3, 3].float().to(dev)
    tanfovx, tanfovy = cam.W / (2 * cam.fx), cam.H / (2 * cam.fy)
    rs = GaussianRasterizationSettings(
        image_height=cam.H, image_width=cam.W, tanfovx=tanfovx, tanfovy=tanfovy,
        bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=view, projmatrix=view,
        sh_degree=3, campos=campos, opaque_threshold=0.6, depth_threshold=1.0,
        normal_threshold=math.cos(math.radians(60.0)), color_sigma=3.0, prefiltered=False, debug=False,
        cx=cam.cx, cy=cam.cy, T_threshold=1e-4)
    rast = GaussianRasterizer(raster_settings=rs)
    tile_mask = torch.ones((cam.H + 15) // 16, (cam.W + 15) // 16, dtype=torch.int32, device=dev)

    gen = torch.Generator().manual_seed(7 + (0 if one_stream else rank))
    gt_color = torch.rand(3, cam.H, cam.W, generator=gen).to(dev)
    poses = synth.trajectory(2, seed=9 + (0 if one_stream else rank))
    base = synth.look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3)
    d0 = synth.box_room_depth(cam, base @ poses[0]).to(dev)
    d1 = synth.box_room_depth(cam, base @ poses[1]).to(dev)
    gt_depth = d1.reshape(1, cam.H, cam.W)
    K = torch.tensor([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=torch.float32, device=dev)
    vp0, np0 = hicp.build_pyramids(d0, K, 3)
    cos_thr = math.cos(math.radians(20.0))

    def render(gd):
        return rast(means3D=gd["xyz"], opacities=gd["opacity"], shs=gd["shs"], colors_precomp=None,
                    scales=gd["scales"], rotations=gd["rotations"], cov3D_precomp=None, normal_w=gd["normal"],
                    tile_mask=tile_mask, grad_rows=gd.get("grad_rows"))

    # Tracking and mapping are independent within a frame (RTG-SLAM runs them as two pipeline stages in separate
    # processes, SLAM/multiprocess/system.py): the tracker's kernels go to a second HIP stream, enqueued by a helper
    # thread - rtg_slam_amd/pipeline.py
    from rtg_slam_amd.pipeline import TrackMapPipeline
    try:
        pipe = TrackMapPipeline(dev, reserve_cus=args.reserve_cus)
    except RuntimeError as e:                # no CU-masked stream on this device / partition mode: run without the reservation
        print(f"bench.py: {e}; running with --reserve-cus 0", file=sys.stderr)
        args.reserve_cus = 0
        pipe = TrackMapPipeline(dev)
    if pipe.mapper_stream is not None:       # everything this thread enqueues from here on: the mapper's masked stream
        pipe.mapper_stream.wait_stream(torch.cuda.current_stream(dev))
        torch.cuda.set_stream(pipe.mapper_stream)

    def track_stage():
        vp1, np1 = hicp.build_pyramids(d1, K, 3)
        return hicp.icp_track(vp1, np1, vp0, np0, K, [0.25, 0.5, 1.0], [5, 5, 5], 0.1, cos_thr, 1e-4)

    # the render mask of the optimisation (mapper.py:500-508: evaluate_render_range renders once before the loop,
    # render_mask = T_map != 1, and hands it to every loss_update) - computed the same way, once, by the HIP producer
    from rtg_slam_amd import slam_ops
    with torch.no_grad():
        gd0 = mo.activate8_hip(opt.state["raw8"]["p"][:N])
        T0 = rast(means3D=opt.state["xyz"]["p"][:N], opacities=gd0["opacity"], shs=opt.state["shs"]["p"][:N].view(N, 16, 3),
                  colors_precomp=None, scales=gd0["scales"], rotations=gd0["rotations"], cov3D_precomp=None,
                  normal_w=gd0["normal"], tile_mask=tile_mask)[6]
    render_mask, _, _ = slam_ops.render_range(T0, 0.5)
    render_mask = render_mask.to(torch.uint8)
    del gd0, T0
    opt.begin_local_optimization()

    # --mode sharded is honoured on one GPU too (the N = 1 anchor of BASELINE configs[4]'s curve: dense gradients,
    # Adam through the autograd path); the other modes collapse to the plain one-call step
    mode = args.mode if (world > 1 or args.mode == "sharded") else "single"

    def loss_fn(gd):
        return mo.slam_losses_hip(render(gd), gt_color, gt_depth, render_mask=render_mask)

    def map_step():
        if mode == "sharded":
            # the north star's literal form: dense gradient reduce-scatter over RCCL, Adam on this rank's N / world
            # rows (optimizer state exists only for them), all-gather of the updated rows
            return opt.step(loss_fn)
        # one C call enqueues the whole iteration; with more than one rank the gradient rows that exist (a few MB
        # instead of 283 MB of dense gradients) are exchanged with in-band counts - no host synchronisation
        return opt.step_slam(rs, gt_color, gt_depth, tile_mask, render_mask=render_mask, tile_band=(mode == "tileband"))

    def frame():
        pipe.track(track_stage)
        loss = map_step()
        return pipe.result(), loss

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    # untimed device pre-warm: a cold box starts at idle clocks and with an empty allocator cache; run the
    # real workload before the W warm-up steps the contract asks for.  The count is FIXED (never
    # time-based): every rank must issue the same number of collectives.
    barrier()
    tc = time.perf_counter()
    frame()
    barrier()
    cold_ms = 1e3 * (time.perf_counter() - tc)                # the very first frame: allocator empty, clocks idle
    # garbage of the set-up is collected NOW - before the pre-warm, not between it and the timed blocks: a collection there
    # idles the GPU for tens of milliseconds and the first block then starts on lowered clocks (measured: 0.455 vs 0.431 ms)
    import gc
    gc.collect()
    gc.freeze()
    for n_pre in range(args.prewarm):
        frame()
        if n_pre % 20 == 19:
            torch.cuda.synchronize(dev)
    for _ in range(args.warmup):
        frame()
    host_ms = []                                              # host time of every frame() call of the timed blocks (diagnostic)
    gc_log = []                                               # (generation, start, seconds) of every collection inside the timed blocks
    def _gc_cb(phase, info):
        if phase == "start":
            gc_log.append([info["generation"], time.perf_counter(), 0.0])
        elif gc_log:
            gc_log[-1][2] = time.perf_counter() - gc_log[-1][1]
    if not os.environ.get("RTGS_BENCH_NO_GC_LOG"):
        gc.callbacks.append(_gc_cb)
    frame_t0 = []                                             # start of every timed frame() call
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        th = time.perf_counter()
        last = frame()
        host_ms.append(1e3 * (time.perf_counter() - th))
        frame_t0.append(th)
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs:
        opt.flush()                                           # every rank: a pending row exchange is collective
        if rank == 0:
            dump_outputs(args.dump_outputs, last, opt, N)

    # the headline: exactly --steps frames, barrier-bracketed, max over ranks
    ms_per_step = 1e3 * dt / args.steps
    frames_per_step = 1 if mode == "tileband" else world
    fps = frames_per_step * 1e3 / ms_per_step
    par = {"single": "1 GPU",
           "sparse": f"dp{world}: replicated map and Adam state, one view per rank, RCCL all-gather of the gradient rows that "
                     "exist (fixed capacity, counts in band, no host sync), identical Adam step on every replica",
           "sharded": f"dp{world}: one view per rank, dense RCCL reduce-scatter of the gradients, Adam on the rank's row "
                      "shard (optimizer state sharded), all-gather of the updated rows",
           "tileband": f"tp{world}: ONE view split into tile bands, loss normalisers all-reduced, sparse gradient-row "
                       "exchange, identical Adam step on every replica"}[mode]
    workload = ("`value` counts UNITS, not SLAM frames (the SLAM frame rate by the reference's definition is "
                "`slam_frames_per_sec`, from the `slam_sequence` leg of --full).  One UNIT per step = 1 ICP track (3 levels x 5 GN "
                "iters, 1200x680, on a second HIP stream) + 1 map-optimisation iteration (raster fwd + masked L1 colour / gated "
                f"depth loss + attach regulariser + raster bwd + fused Adam) over {N} "
                + ("opaque wall discs (single-layer surface map)" if args.surface_map else
                   "random Gaussians (SURVEY.md 8d generator, seed 2024)") +
                ", all tiles.  `value` counts these units; the reference's Replica schedule runs 50 iterations "
                "every 6th frame (~8.3 per frame): see frames_per_sec_replica_schedule")
    if not args.full:
        if rank == 0:
            print(json.dumps({
                "metric": "hot_path_units_per_sec", "value": round(fps, 3), "unit": "units/s", "n_gpus": world,
                "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
                "higher_is_better": True, "scaling": "strong" if mode == "tileband" else "weak", "vs_baseline": None,
                "dtype": "f32", "data": "synthetic",
                "config": {"workload": workload, "gaussians": N, "image": [cam.H, cam.W], "mode": mode, "parallelism": par},
                "cold_first_frame_ms": round(cold_ms, 2), "prewarm_frames": args.prewarm,
                "mapper_reserved_cus": args.reserve_cus, "rccl_ranks": rccl_ranks, "full": False}), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # further timed blocks (same K): the run-to-run spread.  `value` stays the first block.
    block_ms = [ms_per_step]
    for _ in range(max(0, args.repeats - 1)):
        barrier()
        tb = time.perf_counter()
        for _ in range(args.steps):
            th = time.perf_counter()
            frame()
            host_ms.append(1e3 * (time.perf_counter() - th))
            frame_t0.append(th)
        barrier()
        db = time.perf_counter() - tb
        if world > 1:
            t = torch.tensor([db], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            db = float(t.item())
        block_ms.append(1e3 * db / args.steps)

    if _gc_cb in gc.callbacks:
        gc.callbacks.remove(_gc_cb)
    # every host frame over 2 ms: its index, its length, and the garbage collections that ran inside it
    slow_frames = [{"index": i, "ms": round(m, 3),
                    "gc": [[g, round(1e3 * d, 3)] for g, ts, d in gc_log if frame_t0[i] <= ts <= frame_t0[i] + 1e-3 * m]}
                   for i, m in enumerate(host_ms) if m > 2.0][:20]
    # the unit taken apart (same K, world 1 only): what each stage costs on its own THROUGH the same plumbing
    unit_parts = None
    if world == 1:
        def timed(fn):
            for _ in range(5):
                fn()
            barrier()
            tq = time.perf_counter()
            for _ in range(args.steps):
                fn()
            barrier()
            return round(1e3 * (time.perf_counter() - tq) / args.steps, 4)

        def track_via_pipe():
            pipe.track(track_stage)
            return pipe.result()

        def track_direct():
            with torch.cuda.stream(pipe.tracker_stream):
                return track_stage()

        def frame_inline():
            cur = torch.cuda.current_stream(dev)
            pipe.tracker_stream.wait_stream(cur)
            with torch.cuda.stream(pipe.tracker_stream):
                r = track_stage()
            map_step()
            cur.wait_stream(pipe.tracker_stream)
            return r

        unit_parts = {"both_tracker_enqueued_first_by_this_thread_ms": timed(frame_inline),
                      "tracker_only_through_the_pipeline_ms": timed(track_via_pipe),
                      "tracker_only_enqueued_by_this_thread_ms": timed(track_direct),
                      "map_step_only_ms": timed(map_step), "both_ms": timed(frame)}
    opt.flush()
    if pipe.mapper_stream is not None:       # the legs below time the mapper ALONE: back on an unmasked stream
        torch.cuda.synchronize(dev)
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
    # Strong scaling of ONE view (a single SLAM stream has one frame per step): every rank takes a band of the tiles of
    # rank 0's view.  Map iterations only (no tracker), barrier-bracketed, max over ranks.  On one GPU this is the plain
    # map iteration - the number the N > 1 runs are to be compared with.
    strong = None
    if mode != "sharded":
        if world > 1:
            view0 = torch.eye(4, device=dev)
            rs0 = rs._replace(viewmatrix=view0, projmatrix=view0, campos=torch.zeros(3, device=dev))
            gt0 = torch.rand(3, cam.H, cam.W, generator=torch.Generator().manual_seed(7)).to(dev)
        else:
            rs0, gt0 = rs, gt_color
        rm1 = torch.ones(cam.H, cam.W, dtype=torch.uint8, device=dev)
        for _ in range(10):
            opt.step_slam(rs0, gt0, gt_depth, tile_mask, render_mask=rm1, tile_band=world > 1)
        barrier()
        ts = time.perf_counter()
        for _ in range(args.steps):
            opt.step_slam(rs0, gt0, gt_depth, tile_mask, render_mask=rm1, tile_band=world > 1)
        opt.flush()
        barrier()
        dts = time.perf_counter() - ts
        if world > 1:
            t = torch.tensor([dts], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dts = float(t.item())
        strong = {"what": "map-optimisation iterations of ONE 1200x680 view split into tile bands across the ranks "
                          "(sparse gradient-row exchange, loss normalisers all-reduced); no tracker",
                  "n_gpus": world, "ms_per_iteration": round(1e3 * dts / args.steps, 4),
                  "overflow_redos": opt.overflow_redos, "row_capacity": opt._row_capacity}

    # Weak scaling, labelled as such (one view of the sliding window PER RANK; a single SLAM stream cannot produce that many
    # frames at once - tracking is sequential - so this is never `value`): sparse gradient-row exchange, replicated Adam.
    weak = None
    if world > 1 and mode == "tileband":
        c2w_r = synth.look_at_pose(seed=100 + rank, max_angle_deg=2.0, max_trans=0.05)
        view_r = torch.linalg.inv(c2w_r).float().t().contiguous().to(dev)
        rs_r = rs._replace(viewmatrix=view_r, projmatrix=view_r, campos=c2w_r[:3, 3].float().to(dev))
        gt_r = torch.rand(3, cam.H, cam.W, generator=torch.Generator().manual_seed(7 + rank)).to(dev)
        rm1 = torch.ones(cam.H, cam.W, dtype=torch.uint8, device=dev)
        for _ in range(10):
            opt.step_slam(rs_r, gt_r, gt_depth, tile_mask, render_mask=rm1)
        barrier()
        tw = time.perf_counter()
        for _ in range(args.steps):
            opt.step_slam(rs_r, gt_r, gt_depth, tile_mask, render_mask=rm1)
        opt.flush()
        barrier()
        dtw = time.perf_counter() - tw
        t = torch.tensor([dtw], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        weak = {"what": "map iterations with ONE VIEW PER RANK (sparse gradient-row all-gather, identical Adam step on every "
                        "replica); views per second over all ranks - not a SLAM frame rate",
                "n_gpus": world, "ms_per_step": round(1e3 * float(t.item()) / args.steps, 4),
                "views_per_sec": round(world * args.steps / float(t.item()), 2)}

    config5 = None
    if not args.no_config5:
        config5 = config5_block(dev, rank, world, barrier, N=args.config5_gaussians)

    result = None
    if rank == 0:
        lib.rtgs_raster_set_profiling(1)
        prof = profile_scene(lib, mo, rast, opt, N, cam, tile_mask, gt_color, gt_depth, dev, max(3, min(10, args.steps)))
        icp_ms = 0.0
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            vp1, np1 = hicp.build_pyramids(d1, K, 3)
            hicp.icp_track(vp1, np1, vp0, np0, K, [0.25, 0.5, 1.0], [5, 5, 5], 0.1, cos_thr, 1e-4)
            e1.record()
            torch.cuda.synchronize(dev)
            icp_ms += e0.elapsed_time(e1) / 5
        # the op as local_optimize uses it: ~30 % of the tiles switched on
        gyx = tile_mask.numel()
        m30 = torch.zeros(gyx, dtype=torch.int32, device=dev)
        m30[torch.linspace(0, gyx - 1, int(0.3 * gyx)).long().to(dev)] = 1
        prof30 = profile_scene(lib, mo, rast, opt, N, cam, m30.view_as(tile_mask), gt_color, gt_depth, dev, 4)
        # A SURFACE-shaped map of the same size (what RTG-SLAM's mapper builds: one layer of opaque discs on the room's
        # walls, synth.surface_gaussians) - reported beside the headline scene, whose depth complexity the near slice,
        # the row-state backward and the row-skipping Adam exploit
        surface = None
        if not args.no_surface:
            gs = synth.surface_gaussians(N, cam, seed=7)
            opt_s = mo.ShardedMapOptimizer(mo.pack_from_activated({k: v.to(dev) for k, v in gs.items()}),
                                           lr_col=mo.default_lr_columns() * 1e-4)
            gt_d_s = synth.box_room_depth(cam, torch.eye(4, dtype=torch.float64), bump=0.0).to(dev).reshape(1, cam.H, cam.W)
            rm_s = torch.ones(cam.H, cam.W, dtype=torch.uint8, device=dev)
            opt_s.begin_local_optimization()
            for _ in range(20):
                opt_s.step_slam(rs, gt_color, gt_d_s, tile_mask, render_mask=rm_s)
            torch.cuda.synchronize(dev)
            ts = time.perf_counter()
            for _ in range(args.steps):
                opt_s.step_slam(rs, gt_color, gt_d_s, tile_mask, render_mask=rm_s)
            torch.cuda.synchronize(dev)
            map_iter_ms = 1e3 * (time.perf_counter() - ts) / args.steps
            surface = profile_scene(lib, mo, rast, opt_s, N, cam, tile_mask, gt_color, gt_d_s, dev, 5)
            surface["map_iteration_ms"] = round(map_iter_ms, 4)
            # ... and as RTG-SLAM optimises it: most of a mature map is STABLE (rendered, not differentiated, not stepped -
            # mapper.py:1026-1108); here the first 80 % of the rows are frozen, the last 20 % trainable
            opt_u = mo.ShardedMapOptimizer(opt_s.params, lr_col=mo.default_lr_columns() * 1e-4, n_frozen=int(0.8 * N))
            opt_u.begin_local_optimization()
            for _ in range(20):
                opt_u.step_slam(rs, gt_color, gt_d_s, tile_mask, render_mask=rm_s)
            torch.cuda.synchronize(dev)
            tu = time.perf_counter()
            for _ in range(args.steps):
                opt_u.step_slam(rs, gt_color, gt_d_s, tile_mask, render_mask=rm_s)
            torch.cuda.synchronize(dev)
            surface["unstable_20pct"] = {"map_iteration_ms": round(1e3 * (time.perf_counter() - tu) / args.steps, 4),
                                         "trainable_rows": int(opt_u.n_train), "frozen_rows": int(opt_u.n_frozen),
                                         "rows_with_gradient_per_step": int(opt_u.live_counts[0]) // (20 + args.steps)}
            del opt_u
            surface["workload"] = (f"{N} opaque discs on the walls of the 5 x 3 x 6 m box room (one layer, opacity 0.99, radius = "
                                   "sqrt(area / N) clipped to [0.001, 0.05] m), camera inside, all tiles")
            del opt_s
        lib.rtgs_raster_set_profiling(0)
        stage, names, kernels = prof["stage"], prof["names"], prof["kernels"]
        rows_touched, R, consumed, pairs, slice_stats = (prof["rows_touched"], prof["instances"], prof["consumed"],
                                                        prof["pairs"], prof["near_slice"])
        dom, dom_ms, alg = prof["dominant"], prof["dominant_ms"], prof["alg"]
        achieved = alg[dom] / (dom_ms * 1e-3) / 1e9
        # PMC-derived numbers (separate rocprofv3 --pmc passes, tools/measure_round.sh) are only quoted when they were
        # measured on THESE kernel sources: the files carry the hash of rtg_slam_amd/csrc they were collected at.
        traffic, valu = None, None
        src = source_hash()
        dom_pmc = {"blend_bwd": "blend_bwd_entry", "near_slice_blend_fwd": "blend_fwd"}.get(dom, dom)
        same_workload = N == 1_200_000 and not args.surface_map       # the PMC passes ran the default headline workload
        tpath = os.path.join(ROOT, "profiles", "traffic_latest.json")
        if same_workload and os.path.exists(tpath):     # HBM bytes per launch: FETCH_SIZE / WRITE_SIZE, corrected as MI355X_MICROARCH.md prescribes
            try:
                tj = json.load(open(tpath))
                if tj.get("_source_sha16") == src:
                    traffic = (tj.get(dom_pmc) or tj.get(dom) or {}).get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
        vpath = os.path.join(ROOT, "profiles", "valu_latest.json")
        if same_workload and os.path.exists(vpath):     # SQ_INSTS_VALU per launch of the dominant kernel (tools/pmc_sq.py)
            try:
                vj = json.load(open(vpath))
                if vj.get("_source_sha16") == src and dom_pmc in vj:
                    insts = float(vj[dom_pmc]["SQ_INSTS_VALU"])
                    # MEASURED issue peak (tools/probe/valu_rate.hip, profiles/r05_valu_rate.txt): 0.99 G wave64 VALU
                    # instructions / s / SIMD for an FMA stream at 8 waves per SIMD (0.92 at this kernel's 5), by wall clock -
                    # one per ~1.4 shader cycles, not the 4 round 4 assumed nor the 2 the guide implies; DPP instructions
                    # issue at 0.58, v_exp_f32 at 0.29 of that unit
                    peak = 1024 * 0.99e9
                    valu = {"wave_insts_per_launch": int(insts), "achieved_Ginst_s": round(insts / (dom_ms * 1e-3) / 1e9, 1),
                            "peak_Ginst_s": round(peak / 1e9, 1), "frac": round(insts / (dom_ms * 1e-3) / peak, 4),
                            "peak_source": "measured: tools/probe/valu_rate.hip (FMA stream, 8 waves/SIMD, wall clock)",
                            "valu_per_busy_simd_cycle_pmc": vj[dom_pmc].get("valu_per_busy_simd_cycle"),
                            "source": "profiles/valu_latest.json (rocprofv3 --pmc SQ_INSTS_VALU ..., own pass), duration live"}
            except Exception:
                valu = None
        hbm_frac = achieved / HBM_PEAK_GBS
        roofline = {"kernel": dom, "bound": "latency" if valu else "hbm",
                    "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(hbm_frac, 4), "traffic": traffic,
                    "avg_launch_ms": round(dom_ms, 4), "alg_bytes_per_launch": int(alg[dom]), "valu": valu,
                    "frac_blend_fwd_plus_bwd": prof["blend_pair"]["frac"],
                    "frac_blend_fwd_plus_bwd_surface": None if surface is None else surface["blend_pair"]["frac"],
                    "frac_surface": None if surface is None else round(
                        surface["alg"]["blend_bwd"] / (surface["stage"][6] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                    "note": "achieved / peak / frac are the HBM roofline north_star asks for (algorithmic bytes over the live "
                            "launch time).  `bound`: the tile walks reach neither the HBM roofline (~5-8 %) nor, by the probe's FMA "
                            "peak, the VALU one - but SQ counters (profiles/r06_sq_summary_*) show both walks issuing one wave64 VALU "
                            "instruction per ~4.2 cycles per SIMD, the rate of a 16-lane SIMD: they are bound by instruction COUNT "
                            "(round 6: the forward went 79 -> 54 us when its walk loop went from 86 to 50 instructions per step), "
                            "and by the dependent chains per wave that the stamps show (tools/bwd_stamps.py, fwd_stamps.py, "
                            "profiles/r06_*_stamps_*).  traffic / valu are null when profiles/*_latest.json were not measured on "
                            "the current kernel sources or the workload is not the default one", "source_sha16": src}

        cpu = None
        if not args.no_cpu_baseline and world == 1:      # rank 0 at N=1 only
            cpu = cpu_baseline(g, cam, d0, d1, dev)

        # `value` / `ms_per_step`: the first block, exactly --steps frames between barrier + synchronize, max over ranks - the
        # same as a plain run.  Round 6 reported the MEDIAN of the `--repeats` blocks instead: on some machines ONE host frame
        # in ~1 500 takes 8.5-8.7 ms (the same length every time, with or without a short GIL switch interval, with no garbage
        # collection inside it - `host_frames_over_2ms`; on other machines 12 000 frames pass without one), and when it lands
        # in a 20-step block of 8.3 ms it halves that block.  The median stays in the line (`repeats.median_ms_per_step`).
        sched = None
        if world == 1 and not args.no_schedule and not args.no_surface:
            sched = reference_schedule_leg(cam, N, dev)
        seq = None
        if world == 1 and not args.no_sequence:
            seq = sequence_leg(cam, dev, args.sequence_frames)
        tum = icp_tum_leg(dev)
        dropin = None
        if world == 1 and not args.no_dropin:
            dropin = dropin_leg(g, cam, rs, tile_mask, gt_color, gt_depth, render_mask, dev, min(args.steps, 10))
        bs = sorted(block_ms)
        spread = (bs[-1] - bs[0]) / bs[len(bs) // 2]
        result = {
            "metric": "hot_path_units_per_sec", "value": round(fps, 3), "unit": "units/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
            "first_block_ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True, "scaling": "strong" if mode == "tileband" else "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": workload,
                       "gaussians": N, "gaussians_with_gradient": rows_touched, "image": [cam.H, cam.W],
                       "instances": R, "instances_consumed": consumed,
                       "pixel_pairs_evaluated": pairs,
                       "mode": mode, "parallelism": par,
                       # BASELINE.json's metric is three quantities; they live here, where the driver's parser keeps values
                       # (VERDICT r5 "weak 9"): SLAM frames/s by the reference's definition (configs[2], from an empty map),
                       # rasterizer forward + backward at 1.2 M / 1200x680 (volume generator of SURVEY 8d | single-layer surface
                       # map), and the HBM fraction of the two tile walks together (`roofline`)
                       "slam_frames_per_sec": None if seq is None else seq["fps"],
                       "raster_fwd_bwd_ms": round(sum(stage), 4),
                       "raster_fwd_bwd_ms_surface": None if surface is None else surface["raster_fwd_bwd_ms"],
                       "map_iteration_ms": None if unit_parts is None else unit_parts["map_step_only_ms"],
                       "map_iteration_ms_surface": None if surface is None else surface["map_iteration_ms"],
                       "icp_track_ms": round(icp_ms, 4),
                       "icp_track_ms_tum_480x640_noisy": tum["ms_median"],
                       "hbm_frac_blend_fwd_plus_bwd": prof["blend_pair"]["frac"],
                       "config0_cpu_frames_per_sec": None if cpu is None else cpu["config0"]["cpu_frames_per_sec"],
                       "config5_ms_per_iteration": None if config5 is None else config5["ms_per_iteration"]},
            "raster_fwd_ms": round(sum(stage[:6]) + sum(stage[8:10]), 4), "raster_bwd_ms": round(sum(stage[6:8]) + stage[10], 4),
            "raster_fwd_bwd_ms": round(sum(stage), 4), "icp_track_ms": round(icp_ms, 4),
            "raster_fwd_bwd_ms_30pct_tiles": round(sum(prof30["stage"]), 4),
            "cold_first_frame_ms": round(cold_ms, 2), "prewarm_frames": args.prewarm, "mapper_reserved_cus": args.reserve_cus, "unit_parts": unit_parts,
            "unstable": bool(spread > 0.05),
            "repeats": {"blocks": len(block_ms), "spread_over_median": round(spread, 4), "ms_per_step": [round(x, 4) for x in block_ms],
                        "median_ms_per_step": round(bs[len(bs) // 2], 4), "min": round(bs[0], 4), "max": round(bs[-1], 4),
                        "median_frames_per_sec": round(frames_per_step * 1e3 / bs[len(bs) // 2], 2),
                        "host_frames_over_2ms": slow_frames,
                        "slowest_host_frame_ms_per_block": [round(max(host_ms[i:i + args.steps]), 3)
                                                            for i in range(0, len(host_ms), args.steps)]},
            "rccl_ranks": rccl_ranks, "full": True,
            "slam_frames_per_sec": None if seq is None else seq["fps"],
            "slam_sequence": seq,
            "icp_track_ms_tum_480x640_noisy": tum,
            "dropin_iteration_ms": None if dropin is None else dropin["dropin_iteration_ms"],
            "dropin": dropin,
            "config5": config5,
            "weak_scaling_one_view_per_rank": weak,
            "frames_per_sec_replica_schedule": None if sched is None else sched["frames_per_sec"],
            "replica_schedule": sched,
            "strong_scaling_one_view": strong,
            "near_slice": slice_stats, "kernels": kernels, "roofline": roofline, "cpu_baseline": cpu,
            "surface_scene": None if surface is None else {k: surface[k] for k in (
                "workload", "map_iteration_ms", "unstable_20pct", "raster_fwd_ms", "raster_bwd_ms", "raster_fwd_bwd_ms", "instances", "consumed",
                "consumed_fraction", "rows_touched", "near_slice", "kernels")},
        }
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


DUMP_SAMPLE_ROWS = 65536


def dump_outputs(out_dir, last, opt, N):
    """--dump-outputs: what the last timed frame handed its caller, as float32 .npy files (about 16 MB at the default size):
      icp_result       float32[20] of icp_track: the pose (16, row-major) + [valid_ratio, p2p_loss, n_singular, aborted]
      map_loss         the map step's loss (0-dim)
      map_losses       float32[4]: total, colour, depth, ssim (one-call step only; the autograd step of --mode sharded
                       returns the total alone)
      map_{xyz,shs,raw8}_sample: the updated map's rows [:, 3 / 48 / 8] for a FIXED sample of 65 536 rows (seeded; every
      row when the map is smaller); map_sample_rows (float64) holds their indices
    The inputs are seeded, so runs with the same arguments start from identical data.  Two runs of one build agree to
    ~1e-5 relative here; the step's rendered maps are left out: after thousands of steps with float-atomic gradient sums
    ~1 % of their pixels flip a discontinuous decision (depth gate, stop rule) from run to run."""
    import numpy as np
    icp_out, loss = last
    rows = (np.arange(N) if N <= DUMP_SAMPLE_ROWS
            else np.sort(np.random.RandomState(0).choice(N, DUMP_SAMPLE_ROWS, replace=False)))
    idx = torch.from_numpy(rows).to(opt.state["xyz"]["p"].device)
    arrays = {"icp_result": icp_out, "map_loss": loss}
    if opt.last_render is not None:
        arrays["map_losses"] = opt.last_losses
    for nm in ("xyz", "shs", "raw8"):
        arrays[f"map_{nm}_sample"] = opt.state[nm]["p"][:N].index_select(0, idx)
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    host["map_sample_rows"] = rows.astype(np.float64)
    assert sum(a.nbytes for a in host.values()) <= 64 << 20
    os.makedirs(out_dir, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def reference_schedule_leg(cam, N, dev, cycles=3, iters=50, every=6, window=5, n_new=40800):
    """The reference's Replica schedule as a measured workload (slam.py main loop; mapper.py:97-110, 157-205;
    configs/replica_base.yaml:9-18): EVERY frame is preprocessed (tracker.py:97-159), tracked frame-to-model
    (IcpTracker.predict_pose + update_last_status with a render of the map at the new pose), and new Gaussians are added
    where the rendered model is transparent or wrong (temp_points_init's rule with `uniform_sample_num` = 40 800; sample_pixels +
    distCUDA2 radii, gaussian_pointcloud.py:366-405 - the first frame of a run adds all 40 800, later ones what the rule gives); every 6th
    frame the map is optimised: a fresh Adam state (mapper.py:156), evaluate_render_range on each of the 5 window frames
    (one render + T_map -> render / tile masks), then 50 loss_update iterations on a random frame of the window (the last
    frame in the second half, mapper.py:176-183).  1200x680, the 1.2 M single-layer surface map, one GPU, one stream,
    sequential like slam.py, through the product's map object (ShardedMapOptimizer: rows appended every frame, zero-copy
    gaussian_data(), in-place begin_local_optimization).  Dataset IO and the keyframe / stable-set policies are out of scope."""
    import numpy as np
    from types import SimpleNamespace
    from rtg_slam_amd import synth, slam_ops, map_optim as mo
    from rtg_slam_amd.icp import IcpTracker
    from rtg_slam_amd.render import Renderer
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mini_slam as ms
    gs = synth.surface_gaussians(N, cam, seed=7)
    packed = mo.pack_from_activated({k: v.to(dev) for k, v in gs.items()})
    n_frames = every * (cycles + 1)
    base = torch.eye(4, dtype=torch.float64)
    poses = [base @ p for p in synth.trajectory(n_frames, seed=21)]
    K = torch.tensor([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=torch.float32, device=dev)
    frames = []
    for c2w in poses:                                            # "dataset": rendered up front, outside the timed region
        d = synth.box_room_depth(cam, c2w)
        frames.append((d.to(dev), synth.box_room_color(cam, c2w, d).to(dev)))
    tracker, renderer = IcpTracker(ms.ARGS), Renderer(ms.ARGS)
    gen = torch.Generator(device=dev).manual_seed(3)
    rng = np.random.RandomState(5)
    lr = mo.default_lr_columns() * 1e-4          # as in the headline leg: random-ish targets must not inflate the map
    # ONE optimiser for the run (the product's map object): new Gaussians are appended to it every frame, it hands the
    # renderer zero-copy views of its own arrays, and a local optimisation begins by resetting its Adam state in place
    opt = mo.ShardedMapOptimizer(packed, lr_col=lr, capacity=N + 4 * n_new)
    del packed
    state = dict(win=[], c2w=poses[0].clone(), iters=0)
    prof = {} if os.environ.get("RTGS_SCHED_PROFILE") else None     # diagnosis only: per-stage wall time WITH syncs

    def mark(name, t):
        if prof is not None:
            torch.cuda.synchronize(dev)
            if state.get("timed"):                          # the untimed first cycle carries the one-off costs
                prof[name] = prof.get(name, 0.0) + (time.perf_counter() - t)
        return time.perf_counter()

    def one_frame(fid):
        depth, color = frames[fid]
        state["timed"] = fid >= every
        tm_ = time.perf_counter()
        fm = slam_ops.frame_preprocess(depth, K, 0.3, 8.0, False, 0.2)
        tm_ = mark("frame_preprocess", tm_)
        tracker.update_curr_status(fm["depth_map"], K)
        if fid > 0:
            rel, _ = tracker.predict_pose({"K": K, "frame_id": fid})
            state["c2w"] = state["c2w"] @ torch.from_numpy(rel.astype(np.float64))
        tracker.move_last_status()
        tm_ = mark("track", tm_)
        c2w = state["c2w"]
        Rw, tw = c2w[:3, :3].float().to(dev), c2w[:3, 3].float().to(dev)
        vertex_w = fm["vertex_map_c"] @ Rw.t() + tw
        normal_w = fm["normal_map_c"] @ Rw.t()
        view = ms._camera(cam, c2w, dev)
        # gaussians_add (mapper.py:128-132 -> temp_points_init :715-800, configs/base.yaml:47-52): render the model at the new
        # pose; sample transmission_sample_ratio x (uncovered fraction) x uniform_sample_num pixels where the map is
        # transparent (T > add_transmission_thres) and error_sample_ratio x (# pixels) where depth or colour are off; the new
        # Gaussians (radius from the 3 nearest neighbours) are APPENDED to the map - it grows over the run
        with torch.no_grad():
            out = renderer.render(view, opt.gaussian_data())
        T = out["T_map"][0]
        dmap = fm["depth_map"][..., 0]
        depth_ok = dmap > 0
        tmask = (T > 0.5) & depth_ok
        n_trans = int(float(tmask.float().mean()) * 1.0 * n_new)
        cerr = (color - out["render"]).abs().mean(dim=0)
        emask = (((dmap - out["depth"][0]).abs() > 0.1) & depth_ok & (out["depth_index_map"][0] > -1)) | \
                ((cerr > 0.1) & depth_ok & (T < 0.5))
        emask = emask & ~tmask
        n_err = int(float(emask.sum()) * 0.05)
        cmap = color.permute(1, 2, 0).contiguous()
        parts = [slam_ops.sample_pixels(vertex_w, normal_w, cmap, n, m, gen) for n, m in ((n_trans, tmask), (n_err, emask)) if n > 0]
        n_added = sum(int(q[0].shape[0]) for q in parts)
        if n_added >= 4:
            pts, nrm, col = (torch.cat([q[k] for q in parts], 0) for k in range(3))
            opt.append_rows(mo.pack_from_activated(ms.gaussians_from_pixels(pts, nrm, col)))
            state["added"] = state.get("added", 0) + n_added
        tm_ = mark("gaussians_add", tm_)
        rs = ms.renderer_settings(renderer, view, dev)
        state["win"] = (state["win"] + [(rs, color, fm["depth_map"].permute(2, 0, 1).contiguous(), view)])[-window:]
        if (fid + 1) % every == 0 or fid == 0:
            opt.begin_local_optimization()                                     # Adam re-created per local_optimize (in place)
            masks = []
            for (rs_w, _, _, view_w) in state["win"]:                          # evaluate_render_range (mapper.py:471-508)
                with torch.no_grad():
                    out = renderer.render(view_w, opt.gaussian_data())
                rm, tm, _ = slam_ops.render_range(out["T_map"], 0.5)
                masks.append((rm.to(torch.uint8), tm))
            tm_ = mark("optimizer_setup_and_render_range", tm_)
            for it in range(iters):
                j = len(state["win"]) - 1 if it > iters / 2 else int(rng.randint(0, len(state["win"])))
                rs_w, col_w, dep_w, _ = state["win"][j]
                opt.step_slam(rs_w, col_w, dep_w, masks[j][1], render_mask=masks[j][0])
            state["iters"] += iters
            tm_ = mark("map_iterations", tm_)
        with torch.no_grad():                                                  # model depth / normals for the next track
            out = renderer.render(view, opt.gaussian_data())
        tracker.update_last_status(None, out["depth"].permute(1, 2, 0).contiguous(), fm["depth_map"],
                                   out["normal"].permute(1, 2, 0).contiguous(), normal_w)
        mark("model_render_for_tracker", tm_)

    # the legs before this one (the CPU oracle with autograd over a whole frame) leave millions of dead Python objects:
    # a generation-2 collection landing inside the 18 timed frames cost ~95 ms once (71 instead of 110-114 frames/s in
    # one of the round's runs).  Collect now, and keep the survivors out of the collector's way while timing.
    import gc
    gc.collect()
    gc.freeze()
    for fid in range(every):                                                   # one untimed cycle
        one_frame(fid)
    torch.cuda.synchronize(dev)
    it0 = state["iters"]
    t0 = time.perf_counter()
    for fid in range(every, n_frames):
        one_frame(fid)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    gc.unfreeze()
    nf = n_frames - every
    if prof is not None:
        print("schedule leg, ms per frame by stage (with syncs):",
              {k: round(1e3 * v / nf, 3) for k, v in prof.items()}, file=sys.stderr)
    err = float((state["c2w"][:3, 3] - poses[-1][:3, 3]).norm())
    from rtg_slam_amd.rasterizer import current_context
    return {"frames_per_sec": round(nf / dt, 2), "speculation": current_context().speculation_stats(), "ms_per_frame": round(1e3 * dt / nf, 3), "frames": nf,
            "map_iterations": state["iters"] - it0, "iterations_per_frame": round((state["iters"] - it0) / nf, 2),
            "gaussians_start": N, "gaussians_end": int(opt.N), "image": [cam.H, cam.W], "gaussians_appended": int(state.get("added", 0)), "uniform_sample_num": n_new,
            "window": window,
            "final_translation_error_m": round(err, 5),
            "what": "reference Replica schedule (replica_base.yaml: gaussian_update_frame 6, gaussian_update_iter 50, "
                    "memory_length 5, uniform_sample_num 40800), sequential single stream, 1.2 M surface map"}



def sequence_leg(cam, dev, n_frames, seed=21):
    """BASELINE.json configs[2] in the reference's real form, through the product's map object and `Mapping` lifecycle
    (rtg_slam_amd/mapping.py, slam.py): a synthetic Replica-shaped stream (box room, bounded tour: <= 2 cm and <= 1 degree
    per frame), 1200x680, starting from an EMPTY map; per frame preprocess + ICP frame-to-model tracking + gaussians_add;
    every 6th frame evaluate_render_range on the UNSTABLE rows of the 5 window frames and 50 iterations with the stable
    prefix frozen (or, on a keyframe with stable rows, the global optimisation of the stable rows); gaussians_fix at
    confidence > 100, deletion after 120 frames, error counters; reference learning rates (configs/replica_base.yaml).
    `fps` is the reference's number: 1 / mean(mapping seconds per frame) (utils/monitor.py:22-24)."""
    from rtg_slam_amd import mapping as mp, slam, synth
    import gc
    args = mp.replica_args(seed=1)
    poses = synth.room_tour(n_frames, seed=seed)

    def stream():
        for c2w in poses:
            d = synth.box_room_depth(cam, c2w, device=dev)
            c = synth.box_room_color(cam, c2w, d)
            torch.cuda.synchronize(dev)                 # the "dataset read" is over before the frame's clock starts
            yield d.reshape(cam.H, cam.W), c, c2w.numpy()
    torch.cuda.reset_peak_memory_stats(dev)
    gc.collect()
    mapper, tracker, rep = slam.run_sequence(cam, stream(), args, dev, capacity=800_000)
    pf = rep.pop("per_frame")
    opt_frames = [p for i, p in enumerate(pf) if (i + 1) % args.gaussian_update_frame == 0 or i == 0]
    oth_frames = [p for i, p in enumerate(pf) if not ((i + 1) % args.gaussian_update_frame == 0 or i == 0)]
    from rtg_slam_amd.rasterizer import current_context
    out = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in rep.items()}
    out.update({
        "image": [cam.H, cam.W], "start": "empty map", "lr": "reference rates (replica_base.yaml:19-23)",
        "mapping_ms_mean_optimised_frames": round(1e3 * sum(p[1] for p in opt_frames) / max(len(opt_frames), 1), 3),
        "mapping_ms_mean_other_frames": round(1e3 * sum(p[1] for p in oth_frames) / max(len(oth_frames), 1), 3),
        "tracking_ms_mean": round(1e3 * rep["tracking_s_mean"], 3),
        "peak_device_memory_MB": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1),
        "speculation": current_context().speculation_stats(),
        "plain_renders": current_context().plain_stats(),
        "what": "slam.py:56-95 + mapper.py:97-126 on a synthetic Replica-shaped stream (configs[2]); fps = 1 / mean mapping "
                "seconds per frame (utils/monitor.py:22-24); `fps_tracking_plus_mapping` counts the tracker too (single process, "
                "sequential)"})
    return out


def icp_tum_leg(dev, reps=20):
    """BASELINE.json configs[3]: the ICP front-end alone on a TUM fr1-shaped frame pair (640x480, sigma_z noise, 5 % holes,
    1/5000 m quantisation - synth.tum_noise): pyramids of the current frame + 15 Gauss-Newton iterations, HIP events."""
    from rtg_slam_amd import synth, icp as hicp
    cam = synth.TUM_FR1
    poses = synth.trajectory(2, seed=4)
    base = synth.look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3)
    d0 = synth.tum_noise(synth.box_room_depth(cam, base @ poses[0]), seed=1).to(dev).reshape(cam.H, cam.W)
    d1 = synth.tum_noise(synth.box_room_depth(cam, base @ poses[1]), seed=2).to(dev).reshape(cam.H, cam.W)
    K = torch.tensor([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=torch.float32, device=dev)
    vp0, np0 = hicp.build_pyramids(d0, K, 3)
    cos_thr = math.cos(math.radians(20.0))
    ms = []
    for i in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        vp1, np1 = hicp.build_pyramids(d1, K, 3)
        out = hicp.icp_track(vp1, np1, vp0, np0, K, [0.25, 0.5, 1.0], [5, 5, 5], 0.1, cos_thr, 1e-4)
        e1.record()
        torch.cuda.synchronize(dev)
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    host = out.cpu().numpy()
    rel = host[:16].reshape(4, 4)
    gt = (torch.linalg.inv(base @ poses[0]) @ (base @ poses[1])).numpy()
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "image": [cam.H, cam.W],
            "translation_error_m": round(float(((rel[:3, 3] - gt[:3, 3]) ** 2).sum() ** 0.5), 5),
            "what": "pyramids of the new frame + 3 levels x 5 Gauss-Newton iterations + point-to-plane check, TUM fr1 intrinsics, "
                    "noisy depth with holes (configs[3]); frame-to-frame"}


def dropin_leg(g, cam, rs, tile_mask, gt_color, gt_depth, render_mask, dev, steps):
    """What north_star promises the EXISTING Python loop: one iteration of Mapping.loss_update as the reference writes it
    (mapper.py:371-469) - six leaf tensors with torch activations (gaussian_pointcloud.py:16-25, 502-550), the Renderer
    wrapper (SLAM/render.py:60-145; here rtg_slam_amd.render.Renderer, which has the same interface - the reference file
    itself binds unchanged, tests/test_reference_wrapper.py, but /root/reference is not on the GPU box), boolean-mask L1
    colour / depth losses, the attach regulariser, `.backward()`, torch.optim.Adam(lr=0, eps=1e-15) over six groups, the
    confidence update from `_features_dc.grad`, six `.item()` reports, zero_grad - on this package's rasterizer, 1.2 M
    Gaussians, 1200x680.  Beside it the same iteration through the one-call step."""
    import torch.nn as nn
    import torch.nn.functional as F
    from types import SimpleNamespace
    from rtg_slam_amd.render import Renderer
    from rtg_slam_amd import map_optim as mo
    N = g["xyz"].shape[0]
    lrs = [x * 1e-4 for x in (1e-3, 5e-4, 5e-4 / 20.0, 0.0, 4e-3, 1e-3)]        # the headline leg's scaled rates
    P = lambda t: nn.Parameter(t.to(dev).contiguous().requires_grad_(True))
    op = g["opacity"].clamp(1e-6, 1 - 1e-6)
    _xyz, _fdc, _frest = P(g["xyz"]), P(g["shs"][:, :1]), P(g["shs"][:, 1:])
    _opacity, _scaling, _rotation = P(torch.log(op / (1 - op))), P(torch.log(g["scales"])), P(g["rotations"])
    l = [{"params": [p], "lr": lr, "name": n} for p, lr, n in zip((_xyz, _fdc, _frest, _opacity, _scaling, _rotation), lrs,
                                                                   ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"))]
    init = {"opacity": _opacity.detach().clone(), "scaling": _scaling.detach().clone(), "xyz": _xyz.detach().clone(),
            "rotation_raw": _rotation.detach().clone()}
    optimizer = torch.optim.Adam(l, lr=0.0, eps=1e-15)
    confidence = torch.zeros(N, 1, device=dev)
    args = SimpleNamespace(renderer_opaque_threshold=0.6, renderer_normal_threshold=60.0, renderer_depth_threshold=1.0,
                           max_sh_degree=3, color_sigma=3.0, active_sh_degree=3)
    renderer = Renderer(args)
    view = SimpleNamespace(FoVx=2 * math.atan(cam.W / (2 * cam.fx)), FoVy=2 * math.atan(cam.H / (2 * cam.fy)),
                           image_height=cam.H, image_width=cam.W, world_view_transform=rs.viewmatrix,
                           full_proj_transform=rs.projmatrix, camera_center=rs.campos, cx=cam.cx, cy=cam.cy)
    image_input = {"color_map": gt_color.permute(1, 2, 0).contiguous(), "depth_map": gt_depth.permute(1, 2, 0).contiguous()}
    rmask = render_mask.bool()

    def build_rotation(r):                                                     # utils/general_utils.py:108-131
        q = r / torch.sqrt((r * r).sum(dim=1, keepdim=True))
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)

    def gaussian_data():
        scales = torch.exp(_scaling)
        rot = F.normalize(_rotation)
        R = build_rotation(rot)
        idx = torch.argmin(scales, dim=1)
        normal = torch.gather(R.transpose(1, 2), 1, idx.unsqueeze(1).unsqueeze(2).expand(-1, -1, 3))[:, 0, :]
        normal = normal / (torch.norm(normal, p=2, dim=-1, keepdim=True) + 1e-8)
        return {"xyz": _xyz, "opacity": torch.sigmoid(_opacity), "scales": scales, "rotations": rot,
                "shs": torch.cat((_fdc, _frest), dim=1), "normal": normal}

    def loss_update():
        out = renderer.render(view, gaussian_data(), tile_mask=tile_mask)
        attach_mask = (torch.sigmoid(init["opacity"]) < 0.9).squeeze()
        attach_loss = torch.tensor(0)
        if attach_mask.sum() > 0:
            l2 = lambda a, b: ((a - b) ** 2).mean()
            attach_loss = 1000 * (l2(_scaling[attach_mask], init["scaling"][attach_mask]) + l2(_xyz[attach_mask], init["xyz"][attach_mask])
                                  + l2(_rotation[attach_mask], init["rotation_raw"][attach_mask]))
        image, depth, depth_index = out["render"].permute(1, 2, 0), out["depth"].permute(1, 2, 0), out["depth_index_map"].permute(1, 2, 0)
        color_loss = torch.abs(image[rmask] - image_input["color_map"][rmask]).mean()
        depth_error = depth - image_input["depth_map"]
        valid = (depth_index != -1).squeeze() & (image_input["depth_map"] > 0).squeeze() & (depth_error < 0.1).squeeze() & rmask
        depth_loss = torch.abs(depth_error[valid]).mean()
        total = 1.0 * depth_loss + 0.8 * color_loss
        (total + attach_loss).backward()
        optimizer.step()
        grad_mask = (_fdc.grad.abs() != 0).any(dim=-1)
        confidence[grad_mask] += 1
        rep = {"total_loss": total.item(), "depth_loss": depth_loss.item(), "ssim_loss": 0.0, "normal_loss": 0.0,
               "color_loss": color_loss.item(), "scale_loss": attach_loss.item()}
        optimizer.zero_grad(set_to_none=True)
        return rep
    for _ in range(3):
        loss_update()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        rep = loss_update()
    torch.cuda.synchronize(dev)
    ms = 1e3 * (time.perf_counter() - t0) / steps
    touched = int((confidence > 0).sum())
    del optimizer, l
    # the same iteration through the product's one-call step (same map, same rates, same masks)
    opt = mo.ShardedMapOptimizer(mo.pack_from_activated({k: v.to(dev) for k, v in g.items()}), lr_col=mo.default_lr_columns() * 1e-4)
    opt.begin_local_optimization()
    for _ in range(5):
        opt.step_slam(rs, gt_color, gt_depth, tile_mask, render_mask=render_mask)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    for _ in range(steps):
        opt.step_slam(rs, gt_color, gt_depth, tile_mask, render_mask=render_mask)
    torch.cuda.synchronize(dev)
    one = 1e3 * (time.perf_counter() - t1) / steps
    return {"dropin_iteration_ms": round(ms, 3), "one_call_step_ms": round(one, 4), "ratio": round(ms / one, 1),
            "gaussians": N, "gaussians_that_ever_received_gradient": touched, "last_losses": {k: round(v, 6) for k, v in rep.items()},
            "what": "mapper.py:371-469 literally (torch activations, Renderer wrapper, boolean-mask losses, attach term, autograd "
                    "backward with DENSE [N,*] gradients, torch.optim.Adam over six groups, confidence from f_dc.grad, six .item() "
                    "calls) vs ShardedMapOptimizer.step_slam on the same map"}


def config5_block(dev, rank, world, barrier, N=5_000_000, iters=10):
    """BASELINE.json configs[4] as SURVEY.md 8d concretises it: 5 M Gaussians (all unstable), 1200x680, the unstable set
    sharded `world`-way (dense gradient reduce-scatter over RCCL, Adam on the rank's row shard, all-gather of the updated
    rows - ShardedMapOptimizer.step), 10 optimisation iterations, ms per iteration split into render forward (+ loss) /
    render backward / collectives / Adam from HIP events at the phase borders.  One view per rank (the sliding-window form).
    Emitted at every N, including 1 (the anchor of the curve)."""
    from rtg_slam_amd import synth, map_optim as mo
    from rtg_slam_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    cam = synth.REPLICA
    g = synth.random_gaussians(N, cam, seed=2025, z_range=(0.5, 8.0))
    opt = mo.ShardedMapOptimizer(mo.pack_from_activated({k: v.to(dev) for k, v in g.items()}), lr_col=mo.default_lr_columns() * 1e-4)
    del g
    c2w = synth.look_at_pose(seed=100 + rank, max_angle_deg=2.0, max_trans=0.05) if world > 1 else torch.eye(4, dtype=torch.float64)
    view = torch.linalg.inv(c2w).float().t().contiguous().to(dev)
    rs = GaussianRasterizationSettings(
        image_height=cam.H, image_width=cam.W, tanfovx=cam.W / (2 * cam.fx), tanfovy=cam.H / (2 * cam.fy),
        bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=view, projmatrix=view, sh_degree=3,
        campos=c2w[:3, 3].float().to(dev), opaque_threshold=0.6, depth_threshold=1.0,
        normal_threshold=math.cos(math.radians(60.0)), color_sigma=3.0, prefiltered=False, debug=False, cx=cam.cx, cy=cam.cy,
        T_threshold=1e-4)
    rast = GaussianRasterizer(raster_settings=rs)
    gen = torch.Generator().manual_seed(70 + rank)
    gt_c = torch.rand(3, cam.H, cam.W, generator=gen).to(dev)
    gt_d = (0.5 + 4.0 * torch.rand(1, cam.H, cam.W, generator=gen)).to(dev)
    rm = torch.ones(cam.H, cam.W, dtype=torch.uint8, device=dev)

    def loss_fn(gd):
        out = rast(means3D=gd["xyz"], opacities=gd["opacity"], shs=gd["shs"], colors_precomp=None, scales=gd["scales"],
                   rotations=gd["rotations"], cov3D_precomp=None, normal_w=gd["normal"], tile_mask=None, grad_rows=gd.get("grad_rows"))
        return mo.slam_losses_hip(out, gt_c, gt_d, render_mask=rm)
    for _ in range(15):             # the map took seconds of HOST time to generate: the device idled its clocks down meanwhile
        opt.step(loss_fn)
    # VERDICT r5 "weak 5": on a fresh box the FIRST iteration with the phase marks on cost 25 ms of host time (lazy set-up behind
    # the marks' code path) and sat inside the ten timed ones: 3.3 ms per iteration in the driver's line against 0.96 here.  Three
    # untimed iterations WITH the marks now precede the clock, and `ms_per_iteration` is the MEDIAN of the ten (each measured
    # begin -> next begin on the stream); the barrier-bracketed mean stays beside it.
    opt.phase_marks = []
    for _ in range(3):
        opt.step(loss_fn)
    barrier()
    opt.phase_marks = []
    host = []
    t0 = time.perf_counter()
    for _ in range(iters):
        th = time.perf_counter()
        opt.step(loss_fn)
        host.append(1e3 * (time.perf_counter() - th))
    barrier()
    dt = time.perf_counter() - t0
    marks, opt.phase_marks = opt.phase_marks, None
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    begins = [ev for name, ev in marks if name == "begin"]
    ends = [ev for name, ev in marks if name == "end"]
    per_it = [begins[i].elapsed_time(begins[i + 1]) for i in range(len(begins) - 1)] + [begins[-1].elapsed_time(ends[-1])]
    med = sorted(per_it)[len(per_it) // 2]
    if world > 1:
        t = torch.tensor([med], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        med = float(t.item())
    acc = {"render_fwd_and_loss": 0.0, "render_bwd": 0.0, "adam": 0.0, "tail_total": 0.0}
    prev, adam0 = None, None
    for name, ev in marks:
        if name == "forward_and_loss":
            acc["render_fwd_and_loss"] += prev[1].elapsed_time(ev)
        elif name == "backward":
            acc["render_bwd"] += prev[1].elapsed_time(ev)
            bwd_end = ev
        elif name == "adam_begin":
            adam0 = ev
        elif name == "adam_end":
            acc["adam"] += adam0.elapsed_time(ev)
        elif name == "end":
            acc["tail_total"] += bwd_end.elapsed_time(ev)
        if name in ("begin", "forward_and_loss", "backward"):
            prev = (name, ev)
    out = {"gaussians": N, "n_gpus": world, "mode": "sharded", "iterations": iters, "ms_per_iteration": round(med, 3),
           "ms_per_iteration_mean_barrier_bracketed": round(1e3 * dt / iters, 3), "ms_each_iteration": [round(x, 3) for x in per_it],
           "untimed_iterations_before": 15 + 3,
           "split_ms": {"render_fwd_and_loss": round(acc["render_fwd_and_loss"] / iters, 3), "render_bwd": round(acc["render_bwd"] / iters, 3),
                        "collective": round(max(0.0, acc["tail_total"] - acc["adam"]) / iters, 3), "adam": round(acc["adam"] / iters, 3)},
           "host_enqueue_ms_per_iteration": [round(x, 3) for x in host],
           "device_memory_reserved_MB": round(torch.cuda.memory_reserved(dev) / 2 ** 20, 1),
           "dense_gradient_MB_per_rank": round(opt.n_train * 59 * 4 / 1e6, 1),
           "what": "BASELINE configs[4] (SURVEY.md 8d): 5 M Gaussians, 1200x680, unstable set sharded world-way, dense gradient "
                   "reduce-scatter + sharded Adam + all-gather; rank 0's HIP-event split (collective = tail minus Adam, 0 on one GPU)"}
    # The same 5 M map through the SPARSE form (what a SLAM run uses: only the gradient rows that exist travel - a few MB instead
    # of the 1.18 GB dense reduce-scatter + all-gather; replicated Adam state; one C call per iteration)
    packed = opt.params
    del opt
    torch.cuda.empty_cache()
    opt2 = mo.ShardedMapOptimizer(packed, lr_col=mo.default_lr_columns() * 1e-4)
    del packed
    opt2.begin_local_optimization()
    for _ in range(5):
        opt2.step_slam(rs, gt_c, gt_d, None, render_mask=rm)
    opt2.flush()
    barrier()
    t1 = time.perf_counter()
    for _ in range(iters):
        opt2.step_slam(rs, gt_c, gt_d, None, render_mask=rm)
    opt2.flush()
    barrier()
    ds = time.perf_counter() - t1
    if world > 1:
        t = torch.tensor([ds], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ds = float(t.item())
    out["sparse_form_ms_per_iteration"] = round(1e3 * ds / iters, 3)
    out["sparse_form_rows_exchanged_capacity"] = int(opt2._row_capacity) if world > 1 else 0
    del opt2
    torch.cuda.empty_cache()
    return out


def only_leg(args, rank, world, dev):
    """--only <leg>: one extra leg alone (for rocprofv3 runs); prints its JSON on rank 0."""
    from rtg_slam_amd import synth
    cam = synth.REPLICA

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)
    if args.only == "sequence":
        res = sequence_leg(cam, dev, args.sequence_frames)
    elif args.only == "icp_tum":
        res = icp_tum_leg(dev)
    elif args.only == "dropin":
        from rtg_slam_amd.rasterizer import GaussianRasterizationSettings
        g = synth.random_gaussians(args.gaussians, cam, seed=2024)
        eye = torch.eye(4, device=dev)
        rs = GaussianRasterizationSettings(
            image_height=cam.H, image_width=cam.W, tanfovx=cam.W / (2 * cam.fx), tanfovy=cam.H / (2 * cam.fy),
            bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=eye, projmatrix=eye, sh_degree=3,
            campos=torch.zeros(3, device=dev), opaque_threshold=0.6, depth_threshold=1.0,
            normal_threshold=math.cos(math.radians(60.0)), color_sigma=3.0, prefiltered=False, debug=False, cx=cam.cx, cy=cam.cy,
            T_threshold=1e-4)
        tm = torch.ones((cam.H + 15) // 16, (cam.W + 15) // 16, dtype=torch.int32, device=dev)
        gt_c = torch.rand(3, cam.H, cam.W, generator=torch.Generator().manual_seed(7)).to(dev)
        gt_d = synth.box_room_depth(cam, torch.eye(4, dtype=torch.float64), device=dev).reshape(1, cam.H, cam.W)
        rm = torch.ones(cam.H, cam.W, dtype=torch.uint8, device=dev)
        res = dropin_leg(g, cam, rs, tm, gt_c, gt_d, rm, dev, args.steps)
    else:
        res = config5_block(dev, rank, world, barrier, N=args.config5_gaussians)
    if rank == 0:
        print(json.dumps({args.only: res}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def profile_scene(lib, mo, rast, opt, N, cam, tile_mask, gt_color, gt_depth, dev, nprof):
    """Per-stage HIP-event timings (on the launch stream, inside the library), work counters and algorithmic-byte
    rooflines of the rasterizer forward + backward on the optimiser's current map, through the autograd path."""
    counters = torch.zeros(2 * tile_mask.numel(), dtype=torch.int64, device=dev)
    acc = [0.0] * 11
    consumed = pairs = R = 0
    rows_touched = rows_cleared = 0
    slice_stats = None
    for i in range(nprof + 1):                                     # first pass: warm-up AND the work counters (their
        if i == 0:                                                 # per-tile atomics cost blend_fwd ~25 us: not in the timed passes)
            counters.zero_()
            lib.rtgs_raster_set_counters(C.c_void_p(counters.data_ptr()))
        lv = {nm: opt.state[nm]["p"][:N].detach().clone().requires_grad_(True) for nm in ("xyz", "shs", "raw8")}
        opt.grad_rows.begin_step()                                 # same backward as opt.step(): persistent rows + row states
        gd = mo.activate8_hip(lv["raw8"], opt.grad_rows)
        gd["xyz"], gd["shs"] = lv["xyz"], lv["shs"].view(N, 16, 3)
        out = rast(means3D=gd["xyz"], opacities=gd["opacity"], shs=gd["shs"], colors_precomp=None, scales=gd["scales"],
                   rotations=gd["rotations"], cov3D_precomp=None, normal_w=gd["normal"], tile_mask=tile_mask,
                   grad_rows=opt.grad_rows)
        loss = mo.slam_losses_hip(out, gt_color, gt_depth, render_mask=torch.ones_like(gt_depth[0], dtype=torch.uint8))
        lib.rtgs_raster_set_counters(None)
        loss.backward()
        torch.cuda.synchronize(dev)
        if i == 0:
            cc = counters.view(-1, 2).sum(0).cpu()
            consumed, pairs = int(cc[0]), int(cc[1])
            continue
        ms = (C.c_float * 12)()
        lib.rtgs_raster_last_timings(ms)
        for k in range(11):
            acc[k] += max(0.0, ms[k]) / nprof
        sl = (C.c_int64 * 4)()
        lib.rtgs_raster_last_slice_stats(sl)
        slice_stats = {"used": int(sl[0]), "instances": int(sl[1]), "tiles_finished": int(sl[2]),
                       "tiles_left_to_pass2": int(sl[3])}
        st = (C.c_int64 * 8)()
        lib.rtgs_raster_last_stats(st)
        R = int(st[0])
        rows_touched = int((opt.grad_rows.row_state == 1).sum())
        rows_cleared = int((opt.grad_rows.row_state == 2).sum())
    stage = acc
    # With the near-slice pass on, stages 1-5 are the SECOND pass (tiles the slice left unfinished) and 8-9 the slice.
    names = ["preprocess_fwd", "bin_count", "bin_scatter", "bin_tilesort", "tile_ranges_fallback_only",
             "blend_fwd", "blend_bwd", "preprocess_bwd", "near_slice_binning", "near_slice_blend_fwd", "grad_reduce"]
    sliced = bool(slice_stats and slice_stats["used"])
    pass2 = bool(sliced and slice_stats["tiles_left_to_pass2"])
    Px = cam.H * cam.W
    # algorithmic bytes per launch (I := instances the tile walks consume)
    alg = {
        "preprocess_fwd": 248 * N + 64 * N,
        "bin_count": 68 * N,
        "bin_scatter": 68 * N + 8 * R,
        "bin_tilesort": 12 * R,
        "blend_fwd": 68 * consumed + 40 * Px,
        "blend_bwd": 68 * consumed + 28 * Px + 36 * consumed,
        "grad_reduce": N + 64 * consumed + 64 * rows_touched,        # touched bytes + one slot per consumed instance + records
        "preprocess_bwd": 2 * N + (248 + 128 + 236) * rows_touched + 236 * rows_cleared,
    }
    if sliced:
        # geometry-only pre-pass: means + scales + rotations in (40 B), radius x2 + rect area + depth bin + (u, v) out
        alg["preprocess_fwd"] = (40 + 25) * N
        R2 = R - slice_stats["instances"]
        alg["bin_count"] = 68 * N if pass2 else 0
        alg["bin_scatter"] = (68 * N + 8 * R2) if pass2 else 0
        alg["bin_tilesort"] = 12 * R2
        # the tile walks of both passes share the consumed-instance counter: attribute it to the pass that dominates
        if pass2 and stage[5] > stage[9]:
            alg["near_slice_blend_fwd"] = 40 * Px
        else:
            alg["near_slice_blend_fwd"] = alg.pop("blend_fwd")
            if pass2:
                alg["blend_fwd"] = 40 * Px
        # slice: depth bin + rect area + radius per Gaussian (histograms), depth bin per Gaussian twice, 8-B key write +
        # 8-B read + 4-B write per slice instance
        alg["near_slice_binning"] = 9 * N + N + 20 * slice_stats["instances"]
    kernels = {}
    for nm, ms_ in zip(names, stage):
        if nm in alg and ms_ > 0 and alg[nm] > 0:
            kernels[nm] = {"ms": round(ms_, 4), "alg_MB": round(alg[nm] / 1e6, 2), "GBps": round(alg[nm] / (ms_ * 1e-3) / 1e9, 1),
                           "frac_of_hbm_peak": round(alg[nm] / (ms_ * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        else:
            kernels[nm] = {"ms": round(ms_, 4)}
    blend_like = [n for n in names if n in alg and n not in ("near_slice_binning", "grad_reduce") and stage[names.index(n)] > 0]
    dom = max(blend_like, key=lambda n: stage[names.index(n)])
    # the stage brackets carry ~10 us of event overhead each: within 10 % the tile walk of the backward - the kernel the
    # kernel traces (profiles/*_kernel_table.txt) show as the longest - stays the one the roofline is quoted for
    if "blend_bwd" in blend_like and stage[names.index("blend_bwd")] >= 0.9 * stage[names.index(dom)]:
        dom = "blend_bwd"
    # both tile walks together (north_star: ">= 60 % of the HBM roofline on the tile alpha-blend + backward kernels"): the
    # algorithmic bytes of blend_fwd (both passes) + blend_bwd over the sum of their live brackets
    pair_bytes = (68 * consumed + 40 * Px) + (68 * consumed + 28 * Px + 36 * consumed)
    pair_ms = stage[5] + stage[9] + stage[6]
    blend_pair = {"alg_bytes": int(pair_bytes), "ms": round(pair_ms, 4),
                  "GBps": round(pair_bytes / max(pair_ms, 1e-9) / 1e6, 1),
                  "frac": round(pair_bytes / max(pair_ms, 1e-9) / 1e6 / HBM_PEAK_GBS, 4)}
    return {"stage": stage, "names": names, "kernels": kernels, "alg": alg, "dominant": dom, "blend_pair": blend_pair,
            "dominant_ms": stage[names.index(dom)], "instances": R, "consumed": consumed, "pairs": pairs,
            "consumed_fraction": round(consumed / max(R, 1), 4), "rows_touched": rows_touched, "near_slice": slice_stats,
            "raster_fwd_ms": round(sum(stage[:6]) + sum(stage[8:10]), 4), "raster_bwd_ms": round(sum(stage[6:8]) + stage[10], 4),
            "raster_fwd_bwd_ms": round(sum(stage), 4)}


def cpu_baseline(g, cam, d0, d1, dev):
    """The oracle (PyTorch-CPU restatement; the reference has no CPU render path and its rasterizer source is absent)
    on the host cores.  Two legs:
      * `value`: the SAME unit as `value` of the bench line, MEASURED, nothing scaled: rasterizer forward + backward of
        the whole 1.2 M / 1200x680 frame (oracle/raster_oracle_fast.py: raster_oracle's per-Gaussian stage and binning,
        the tile blend and its hand-written backward over all tiles - the form the whole-image parity test uses) plus
        one full-size ICP track with the pinned ICP oracle; about 30-40 s of CPU (nothing extrapolated).
      * `config2_measured`: BASELINE.json configs[1] (200 000 Gaussians, 640x480, all tiles, forward + backward)
        through raster_oracle.py + autograd, next to the HIP time for the very same call."""
    from oracle import raster_oracle as ro
    from oracle import raster_oracle_fast as rf
    from oracle import icp_oracle as io
    from rtg_slam_amd import synth
    threads = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(threads)
    N = g["xyz"].shape[0]
    s = ro.make_settings(cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy)
    gy, gx = (cam.H + 15) // 16, (cam.W + 15) // 16
    ones_c, ones_d = torch.ones(3, cam.H, cam.W), torch.ones(1, cam.H, cam.W)
    t0 = time.perf_counter()
    rf.forward_backward(s, g["xyz"], g["opacity"], g["shs"], g["scales"], g["rotations"], g["normal"], None, ones_c, ones_d)
    raster_full = time.perf_counter() - t0
    K = torch.tensor([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=torch.float32)
    ti0 = time.perf_counter()
    vp0 = io.vertex_pyramid(d0.cpu(), K.clone(), 3); np0 = io.normal_pyramid(vp0)
    vp1 = io.vertex_pyramid(d1.cpu(), K.clone(), 3); np1 = io.normal_pyramid(vp1)
    io.track(vp1, np1, vp0, np0, K.clone())
    icp_s = time.perf_counter() - ti0
    # ---- configs[1], measured end to end, no scaling: CPU oracle vs the HIP op on the same tensors
    c2 = synth.CONFIG2
    g2 = synth.random_gaussians(200_000, c2, seed=2024)
    s2 = ro.make_settings(c2.H, c2.W, c2.fx, c2.fy, c2.cx, c2.cy)
    gen = torch.Generator().manual_seed(11)
    gc, gd = torch.randn(3, c2.H, c2.W, generator=gen), torch.randn(1, c2.H, c2.W, generator=gen)
    lv = {k: v.clone().requires_grad_(True) for k, v in g2.items()}
    tc = time.perf_counter()
    o2 = ro.rasterize(s2, lv["xyz"], lv["opacity"], lv["shs"], lv["scales"], lv["rotations"], lv["normal"], None)
    ((o2[0] * gc).sum() + (o2[1] * gd).sum()).backward()
    c2_cpu = time.perf_counter() - tc
    from tests import raster_util as ru
    from diff_gaussian_rasterization_depth import GaussianRasterizer
    rast2 = GaussianRasterizer(raster_settings=ru.hip_settings(s2, dev))
    gl = {k: v.to(dev) for k, v in g2.items()}
    gcd, gdd = gc.to(dev), gd.to(dev)
    ms = []
    for i in range(8):
        lh = {k: v.clone().requires_grad_(True) for k, v in gl.items()}
        torch.cuda.synchronize(dev)
        th = time.perf_counter()
        oh = rast2(means3D=lh["xyz"], opacities=lh["opacity"], shs=lh["shs"], colors_precomp=None, scales=lh["scales"],
                   rotations=lh["rotations"], cov3D_precomp=None, normal_w=lh["normal"], tile_mask=None)
        ((oh[0] * gcd).sum() + (oh[1] * gdd).sum()).backward()
        torch.cuda.synchronize(dev)
        ms.append(1e3 * (time.perf_counter() - th))
    c2_gpu_ms = sorted(ms[2:])[len(ms[2:]) // 2]
    c2_err = float((oh[0].detach().cpu() - o2[0].detach()).abs().max())
    config0 = config0_block(cam, dev)
    return {"value": round(1.0 / (raster_full + icp_s), 5), "unit": "units/s", "cores": threads, "kind": "port", "config0": config0,
            "extrapolated": False,
            "threads_by_stage": {"per_gaussian_stage_and_autograd": threads, "tile_blend_loop": min(threads, 4), "icp": threads},
            "note": "measured, nothing scaled; the tile loop of the oracle caps torch's intra-op threads at 4 (its tensors are "
                    "[<= 128, 256]: more threads are slower), the per-Gaussian stage and the ICP use `cores`.  The reference's "
                    "own CPU ICP (SLAM/icp.py) cannot run on this box (no /root/reference here) - oracle/icp_oracle.py is "
                    "pinned to its outputs at this size by tests/golden/icp_full_*.npz and stands in",
            "sample": f"ONE unit of the workload: oracle raster fwd+bwd of all {N} Gaussians on all {gy * gx} tiles "
                      f"({raster_full:.1f} s) + 1 full-size ICP track incl. pyramids ({icp_s:.2f} s); no loss / Adam term on "
                      "the CPU side",
            "measured_s": round(raster_full + icp_s, 2),
            "config2_measured": {"workload": "BASELINE.json configs[1]: 200000 Gaussians, 640x480, all tiles, rasterizer "
                                             "forward + backward, random upstream gradients, nothing scaled",
                                 "cpu_oracle_s": round(c2_cpu, 2), "hip_ms": round(c2_gpu_ms, 3),
                                 "speedup": round(1e3 * c2_cpu / c2_gpu_ms, 1), "max_abs_color_diff": c2_err}}


def config0_block(cam_full, dev, frames=50, down=4, n_gaussians=60_000):
    """BASELINE.json configs[0]: "first 50 frames, GT poses, PyTorch-CPU render path (no GPU, plumbing reference)" - the loop of
    /root/reference/slam.py:56-95 with `use_gt_pose` (configs/replica/replica_base.yaml:26-31) reduced to what it renders: every
    frame of a synthetic Replica-shaped stream is rendered AT ITS GROUND-TRUTH POSE through the repository's PyTorch-CPU
    render path (oracle/raster_oracle.py; the reference has none - BASELINE.md section 3) from a fixed single-layer map and
    compared with the frame.  Sized for ~30-60 s of host time: 50 frames at a QUARTER of the Replica resolution (170x300),
    60 000 wall discs.  The same 50 renders through the HIP forward stand beside it.  Part of the cpu_baseline leg (the only
    place bench.py may touch oracle/)."""
    from oracle import raster_oracle as ro
    from rtg_slam_amd import synth
    from tests import raster_util as ru
    from diff_gaussian_rasterization_depth import GaussianRasterizer
    c = cam_full
    cam = synth.CameraSpec(c.H // down, c.W // down, c.fx / down, c.fy / down, (c.cx + 0.5) / down - 0.5, (c.cy + 0.5) / down - 0.5)
    g = synth.surface_gaussians(n_gaussians, cam, seed=7)
    gl = {k: v.to(dev) for k, v in g.items()}
    poses = synth.trajectory(frames, seed=5)
    cpu_s, hip_ms, psnr, dl1, worst = 0.0, [], [], [], 0.0
    for c2w in poses:
        depth = synth.box_room_depth(cam, c2w, bump=0.0)
        color = synth.box_room_color(cam, c2w, depth)
        view = torch.linalg.inv(c2w).float().t().contiguous()
        s = ro.make_settings(cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy, viewmatrix=view, campos=c2w[:3, 3].float())
        t0 = time.perf_counter()
        with torch.no_grad():
            out = ro.rasterize(s, g["xyz"], g["opacity"], g["shs"], g["scales"], g["rotations"], g["normal"])
        cpu_s += time.perf_counter() - t0
        covered = out[6][0] < 0.5
        mse = float(((out[0] - color) ** 2)[:, covered].mean())
        hit = covered & (out[1][0] > 0)
        psnr.append(10 * math.log10(1.0 / max(mse, 1e-12)))
        dl1.append(float((out[1][0] - depth[..., 0]).abs()[hit].mean()))
        rast = GaussianRasterizer(raster_settings=ru.hip_settings(s, dev))
        for rep in range(2):            # the second call is the timed one (the first sizes the context's buffers for this view)
            torch.cuda.synchronize(dev)
            th = time.perf_counter()
            with torch.no_grad():
                oh = rast(means3D=gl["xyz"], opacities=gl["opacity"], shs=gl["shs"], colors_precomp=None, scales=gl["scales"],
                          rotations=gl["rotations"], cov3D_precomp=None, normal_w=gl["normal"], tile_mask=None)
            torch.cuda.synchronize(dev)
        hip_ms.append(1e3 * (time.perf_counter() - th))
        worst = max(worst, float((oh[0].cpu() - out[0]).abs().max()))
    return {"frames": frames, "image": [cam.H, cam.W], "gaussians": n_gaussians, "poses": "ground truth",
            "cpu_frames_per_sec": round(frames / cpu_s, 3), "cpu_seconds": round(cpu_s, 2),
            "hip_forward_frames_per_sec": round(1e3 * frames / sum(hip_ms), 1),
            "psnr_mean_db": round(sum(psnr) / frames, 2), "depth_l1_mean_m": round(sum(dl1) / frames, 5),
            "max_abs_colour_diff_hip_vs_cpu": worst,
            "what": "BASELINE configs[0]: 50 frames of a synthetic Replica-shaped stream rendered at their GT poses through the "
                    "PyTorch-CPU render path (oracle/raster_oracle.py), quarter resolution so that the leg fits a minute of "
                    "host time; the HIP forward on the same frames beside it (host-synchronised per frame)"}


if __name__ == "__main__":
    main()
