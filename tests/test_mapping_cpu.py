"""Host logic of rtg_slam_amd.mapping.Mapping on the CPU (torch doubles for every kernel, tests/mapping_doubles.py): the
map's lifecycle through a short synthetic stream - add on an EMPTY map, local optimisation with masks from the UNSTABLE
rows, fix by confidence, delete by age, attach, error counters, keyframes, the keyframe-triggered and the final global
optimisation - against what mapper.py:97-126, 134-210, 253-335, 471-592, 594-707 prescribe."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import slam_ops_oracle as so  # noqa: E402
from rtg_slam_amd import synth, mapping as mp  # noqa: E402
from tests.mapping_doubles import TorchOps  # noqa: E402

CAM = synth.CameraSpec(48, 64, 40.0, 40.0, 31.5, 23.5)


def _stream(n, seed=4):
    base = torch.eye(4, dtype=torch.float64)
    poses = [base @ p for p in synth.trajectory(n, seed=seed)]
    out = []
    for c2w in poses:
        d = synth.box_room_depth(CAM, c2w)
        out.append((d, synth.box_room_color(CAM, c2w, d), c2w))
    return out


def _changing_stream(n, seed=4):
    """The stream above with a scene CHANGE from frame 2 on: a patch of the view comes 0.25 m closer and one moves 0.3 m away (the stable
    Gaussians there collect depth-error strikes until error_gaussians_remove deletes them, mapper.py:560-575) and another patch
    changes colour (colour-error strikes until they are released, :576-592)."""
    out = []
    for fid, (d, c, c2w) in enumerate(_stream(n, seed)):
        if fid >= 2:
            d = d.clone()
            d[8:26, 6:26] -= 0.25                                    # [H, W, 1]
            d[30:44, 6:26] += 0.3                                    # ... and one moves away
            c = synth.box_room_color(CAM, c2w, d)
            c[:, 28:44, 36:60] = (c[:, 28:44, 36:60] + 0.5) % 1.0
        out.append((d, c, c2w))
    return out


def _frame_map(depth, color, frame, args):
    K = frame.K
    fm = so.frame_preprocess(depth.reshape(CAM.H, CAM.W, 1), K, args.min_depth, 8.0, False, args.invalid_confidence_thresh)
    c2w = frame.get_c2w
    fm["color_map"] = color.permute(1, 2, 0).contiguous()
    fm["vertex_map_w"] = fm["vertex_map_c"] @ c2w[:3, :3].T + c2w[:3, 3]
    fm["normal_map_w"] = fm["normal_map_c"] @ c2w[:3, :3].T
    return fm


def _args(**kw):
    base = dict(uniform_sample_num=260, gaussian_update_iter=4, gaussian_update_frame=2, memory_length=3,
                stable_confidence_thres=2.0, unstable_time_window=3, max_depth=8.0, keyframe_trans_thes=0.015,
                final_global_iter=2, seed=3)
    base.update(kw)
    return mp.replica_args(**base)


def _args_tum(**kw):
    """The same reduced schedule on configs/tum_base.yaml's values (feature_lr 0.001, scaling_lr 0.02, the *_lr_coef 1.0)."""
    base = dict(uniform_sample_num=260, gaussian_update_iter=4, gaussian_update_frame=2, memory_length=3,
                stable_confidence_thres=2.0, unstable_time_window=3, max_depth=8.0, keyframe_trans_thes=0.015,
                final_global_iter=2, seed=3)
    base.update(kw)
    return mp.tum_args(**base)


def _args_scannetpp(**kw):
    """The reduced schedule on the Scannetpp dataset type: every optimised frame runs the local optimisation and - on a
    keyframe - the global one too (mapper.py:107-113), and the loss leaves out the pixels without depth (:419-420)."""
    return _args(type="Scannetpp", **kw)


def _run(n_frames, args, final=False):
    ops = TorchOps(args)
    m = mp.Mapping(args, torch.device("cpu"), ops=ops, capacity=400)
    log = []
    for fid, (d, c, c2w) in enumerate(_stream(n_frames)):
        fr = mp.Frame(CAM, c2w, torch.device("cpu"), uid=fid)
        fm = _frame_map(d, c, fr, args)
        before = (m.opt.N, m.opt.n_frozen)
        p_stable = m.opt.params[:m.opt.n_frozen].clone()
        n_steps = len(ops.steps)
        m.mapping(fr, fm, fid)
        m.get_render_output(fr)
        log.append(dict(fid=fid, before=before, after=(m.opt.N, m.opt.n_frozen), stable_before=p_stable,
                        steps=ops.steps[n_steps:], stats=dict(m.stats)))
        m.time += 1
    if final:
        m.global_optimization(select_keyframe_num=-1, is_end=True)
    return m, ops, log


def test_lifecycle_from_an_empty_map():
    args = _args()
    m, ops, log = _run(7, args)
    o = m.opt
    tiles = ((CAM.H + 15) // 16) * ((CAM.W + 15) // 16)
    # frame 0: an empty map takes uniform_sample_num pixels (minus those update_geometry drops), all unstable, and is optimised
    assert log[0]["before"] == (0, 0) and 150 < log[0]["stats"]["added"] <= args.uniform_sample_num
    assert len(log[0]["steps"]) == args.gaussian_update_iter
    assert all(s[0] == log[0]["stats"]["added"] and s[1] == 0 for s in log[0]["steps"])
    # optimised frames: time 0 and every gaussian_update_frame-th (mapper.py:103)
    assert m.optimize_frames_ids == [0, 1, 3, 5]
    assert [bool(l["steps"]) for l in log] == [True, True, False, True, False, True, False]
    # confidence counts optimisation hits; above the threshold a Gaussian turns stable
    assert m.stats["fixed"] > 0 and o.n_frozen > 0 and log[0]["after"][1] > 0
    # frame 1 is no keyframe: LOCAL optimisation - the whole map rendered, training starts behind the stable prefix, and the
    # tile masks come from a render of the UNSTABLE rows alone (a few tiles, not all 12)
    nf1 = log[1]["before"][1]
    assert nf1 > 0 and all(s[1] == nf1 and s[0] > nf1 and 0 < s[2] < tiles for s in log[1]["steps"])
    # frames 3 and 5 moved far enough to be keyframes with stable rows present: GLOBAL optimisation - only the stable rows
    # are rendered, trained from row 0, on the 40 % of the tiles with the largest colour error (mapper.py:477-496)
    assert m.keyframe_ids == [0, 3, 5] and m.stats["global_opts"] == 2 and m.stats["local_opts"] == 2
    for l in (log[3], log[5]):
        nf = l["before"][1]
        assert all(s == (nf, 0, int(tiles * 0.4), int(tiles * 0.4) * 256) for s in l["steps"])
        assert l["after"][0] > nf                                            # the unstable rows exist, and were left out
    assert m.opt._scope == "local"
    # unstable Gaussians older than the window are gone (mapper.py:309-311)
    age = m.time - 1 - o.aux["add_tick"][o.n_frozen:o.N, 0]
    assert o.n_train > 0 and int(age.max()) <= args.unstable_time_window and m.stats["deleted_unstable"] > 0
    # error_gaussians_remove and get_render_output share one render when nothing was deleted in between
    assert m.stats["renders_reused"] > 0
    # new points that project onto a stable Gaussian and lie on its plane start at opacity 0.1 (mapper.py:830-883)
    op = torch.sigmoid(o.state["raw8"]["p"][:o.N, 0])
    assert int(((op - 0.1).abs() < 1e-4).sum()) > 0 and bool((op[:log[0]["after"][1]] > 0.9).all())


def test_stable_rows_do_not_move_in_a_local_optimisation_and_masks_come_from_the_unstable_rows():
    args = _args(keyframe_trans_thes=10.0, keyframe_theta_thes=400.0)       # never a keyframe: every optimisation is local
    m, ops, log = _run(4, args)
    assert m.stats["global_opts"] == 0 and m.stats["local_opts"] == 3
    # fixed Gaussians carry a confidence clipped to the threshold (mapper.py:268-270; only a global optimisation raises it again)
    assert m.opt.n_frozen > 0 and float(m.opt.aux["confidence"][:m.opt.n_frozen].max()) <= args.stable_confidence_thres
    l = log[3]                                                               # optimised at time 3 with stable rows present
    nf = l["before"][1]
    assert nf > 0 and l["steps"]
    assert all(s[1] >= nf for s in l["steps"])                               # trainable range behind the stable prefix
    # the stable rows the frame started with are still the first rows, bit for bit (fix only appends behind them)
    assert torch.equal(m.opt.params[:nf], l["stable_before"])
    # a fresh render of the unstable rows alone gives exactly the masks evaluate_render_range handed the steps
    fr = m.processed_frames[-1]
    rm, tm, _ = m.evaluate_render_range(fr)
    full = ops.render(fr, m.opt.gaussian_data("all"))
    assert int(tm.sum()) <= int(ops.render_range(full["T_map"], 0.5)[1].sum())


def test_keyframe_triggers_a_global_optimisation_of_the_stable_rows_only():
    args = _args(keyframe_trans_thes=0.0)                                    # every optimised frame after the first is a keyframe
    m, ops, log = _run(6, args)
    assert m.keyframe_ids == [0, 1, 3, 5] and m.stats["global_opts"] == 3 and m.stats["local_opts"] == 1
    k = int(((CAM.H + 15) // 16) * ((CAM.W + 15) // 16) * 0.4)
    for l in (log[1], log[3], log[5]):
        nf = l["before"][1]
        assert nf > 0 and len(l["steps"]) == args.gaussian_update_iter
        assert all(s == (nf, 0, k, k * 256) for s in l["steps"])             # stable rows only, top-40 % colour-error tiles
        # the unstable rows of that frame were neither rendered nor stepped: bit-unchanged through the optimisation is
        # covered by tests/test_map_object_cpu.py; here: they are still there afterwards
        assert l["after"][0] > nf
    assert m.opt._scope == "local"


def test_final_global_optimisation_fixes_everything_first():
    args = _args()
    m, ops, log = _run(3, args, final=True)
    assert m.opt.n_train == 0 and m.opt.n_frozen == m.opt.N > 0
    n_final = m.get_keyframe_num * args.final_global_iter
    last = ops.steps[-n_final:]
    assert all(s[0] == m.opt.N and s[1] == 0 and s[2] is None for s in last)  # all rows, no tile mask (mapper.py:497-499)
    assert m.weights.depth_weight == 0.0                                     # update_args.depth_weight = 0 (mapper.py:633)


def test_save_model_writes_the_reference_snapshot_files(tmp_path):
    """Mapping.save_model (mapper.py:916-941): unstable / stable / merged clouds with and without the confidence column,
    readable back (io_formats.load_model_ply) to the map's own rows."""
    from rtg_slam_amd import io_formats as iof
    args = _args()
    m, ops, log = _run(3, args)
    o = m.opt
    assert o.n_frozen > 0 and o.n_train > 0
    base = str(tmp_path / "iter_0000")
    m.save_model(base)
    for suffix in ("", "_stable", "_merge", "_sibr", "_stable_sibr", "_merge_sibr"):
        assert os.path.exists(base + suffix + ".ply"), suffix
    st, un, me = iof.load_model_ply(base + "_stable.ply"), iof.load_model_ply(base + ".ply"), iof.load_model_ply(base + "_merge.ply")
    P = o.params.numpy()
    assert st["xyz"].shape[0] == o.n_frozen and un["xyz"].shape[0] == o.n_train and me["xyz"].shape[0] == o.N
    assert np.array_equal(iof.model_to_packed(st), P[:o.n_frozen]) and np.array_equal(iof.model_to_packed(un), P[o.n_frozen:])
    assert np.array_equal(st["confidence"].reshape(-1), o.aux["confidence"][:o.n_frozen, 0].numpy())
    names, _ = iof._read_ply_table(base + "_sibr.ply")                      # the viewer's files carry no confidence column
    assert "confidence" not in names and "confidence" in iof._read_ply_table(base + ".ply")[0]


def _against_the_references_own_mapping(golden, stream_fn, every_frame, args_fn=None):
    """tests/golden/mapping_ref.npz holds the states of the reference's OWN Mapping (SLAM/multiprocess/mapper.py with its
    gaussian_pointcloud.py / render.py / utils.py, run on the CPU from /root/reference by oracle/gen_mapping_golden.py) after
    every frame of this file's stream: gaussians_add on an empty map, local optimisations, two keyframe-triggered global
    optimisations, fixes, deletions, error counters, and after the final global optimisation of slam.py:129.  Both sides use the same oracle rasterizer / k-NN / error accumulation
    and the same random streams, so what is compared is the lifecycle itself: the sizes of both clouds EXACTLY, every raw
    tensor of every Gaussian to float tolerance (the reference steps torch.optim.Adam over six tensors, this package its
    block-SoA Adam: same arithmetic, different summation order in the loss), the optimised frames and the keyframes."""
    import random
    ref = np.load(os.path.join(ROOT, "tests", "golden", golden))
    n_frames, seed = int(ref["n_frames"][0]), int(ref["seed"][0])
    args = (args_fn or _args)()
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    ops = TorchOps(args)
    ops.gen = None                               # torch's default generator, as SLAM/utils.py:173 uses it
    m = mp.Mapping(args, torch.device("cpu"), ops=ops, capacity=600)
    m.rng = random                               # python's global stream, as mapper.py:178, 682
    worst = 0.0

    def compare(tag_prefix):
        nonlocal worst
        o = m.opt
        nu, ns = (int(v) for v in ref[f"{tag_prefix}_sizes"])
        assert (o.N - o.n_frozen, o.n_frozen) == (nu, ns), (tag_prefix, (o.N - o.n_frozen, o.n_frozen), (nu, ns))
        P = o.params[:o.N]
        for tag, r0, r1 in (("s", 0, o.n_frozen), ("u", o.n_frozen, o.N)):
            if r1 == r0:
                continue
            mine = {"xyz": P[r0:r1, 0:3], "f_dc": P[r0:r1, 3:6].reshape(-1, 1, 3), "f_rest": P[r0:r1, 6:51].reshape(-1, 15, 3),
                    "opacity": P[r0:r1, 51:52], "scaling": P[r0:r1, 52:55], "rotation": P[r0:r1, 55:59],
                    "confidence": o.aux["confidence"][r0:r1], "add_tick": o.aux["add_tick"][r0:r1],
                    "depth_error_counter": o.aux["depth_error_counter"][r0:r1], "color_error_counter": o.aux["color_error_counter"][r0:r1]}
            order_m = order_w = None
            if not every_frame:
                # the reference RE-APPENDS a released Gaussian to the end of the stable cloud (mapper.py:286-295), this package
                # leaves the row where it is: same rows, another order - compared in the order of their positions
                key = lambda x: np.lexsort(np.round(x.numpy().astype(np.float64), 3).T[::-1])
                order_m = torch.from_numpy(key(mine["xyz"]))
                order_w = torch.from_numpy(key(torch.from_numpy(ref[f"{tag_prefix}_{tag}_xyz"])))
            for k, v in mine.items():
                want = torch.from_numpy(ref[f"{tag_prefix}_{tag}_{k}"]).to(v.dtype)
                assert want.shape == v.shape, (tag_prefix, tag, k, want.shape, v.shape)
                if order_m is not None:
                    v, want = v[order_m], want[order_w]
                if k in ("confidence", "add_tick", "depth_error_counter", "color_error_counter"):
                    assert torch.equal(v, want), (tag_prefix, tag, k)
                else:
                    err = float((v - want).abs().max())
                    worst = max(worst, err)
                    assert err < 2e-4, (tag_prefix, tag, k, err)

    for fid, (d, c, c2w) in enumerate(stream_fn(n_frames)):
        fr = mp.Frame(CAM, c2w, torch.device("cpu"), uid=fid)
        m.mapping(fr, _frame_map(d, c, fr, args), fid)
        m.get_render_output(fr)
        o = m.opt
        assert (o.N - o.n_frozen, o.n_frozen) == tuple(int(v) for v in ref[f"f{fid}_sizes"]), fid
        if every_frame or fid == n_frames - 1:
            compare(f"f{fid}")
        m.time += 1
    assert m.optimize_frames_ids == ref["optimize_frames_ids"].tolist()
    assert m.keyframe_ids == ref["keyframe_ids"].tolist()
    m.global_optimization(select_keyframe_num=-1, is_end=True)           # slam.py:129
    compare("final")
    print(golden, "- largest difference to the reference's own Mapping over the stream:", worst)
    return m


def test_lifecycle_matches_the_references_own_mapping():
    _against_the_references_own_mapping("mapping_ref.npz", _stream, True)


def test_lifecycle_matches_the_references_own_mapping_with_the_tum_rates():
    """The 7-frame stream with configs/tum_base.yaml's learning rates and coefficients: pins the learning-rate columns of the
    local, the keyframe-triggered and the final global optimisation for the second argument set."""
    _against_the_references_own_mapping("mapping_ref_tum.npz", _stream, True, _args_tum)


def test_lifecycle_matches_the_references_own_mapping_on_the_scannetpp_branch():
    """The 7-frame stream with args.type = "Scannetpp": local + keyframe-triggered global optimisation in ONE frame, loss mask
    without the depth-less pixels of the image the step is given."""
    _against_the_references_own_mapping("mapping_ref_scannetpp.npz", _stream, True, _args_scannetpp)


def test_lifecycle_matches_the_references_own_mapping_with_the_normal_term():
    """normal_weight 0.2 (0.0 in every configuration file of the reference, so this is the only place the term is held to
    mapper.py:433-443): the 7-frame stream again, every parameter within 2e-4."""
    _against_the_references_own_mapping("mapping_ref_normal.npz", _stream, True, lambda: _args(normal_weight=0.2))


def test_lifecycle_matches_the_references_own_mapping_on_a_changing_scene():
    """Fifteen frames with a scene change from frame 2 on (_changing_stream): colour-error strikes release stable Gaussians
    (confidence 0, new tick - mapper.py:576-592), a large fix at frame 11, six keyframes; sizes after every frame, all
    tensors and counters after the last one and after the final global optimisation."""
    m = _against_the_references_own_mapping("mapping_ref_changing.npz", _changing_stream, False)
    assert m.stats["released"] > 0


def test_update_poses_and_the_small_accessors():
    """mapper.py:134-141 (poses corrected by a back end reach the window's frames and the keyframes, and invalidate their
    cached renders), :286-295 (release), :1116-1134 (counters)."""
    args = _args()
    m, ops, log = _run(4, args)
    assert m.get_total_num == m.get_stable_num + m.get_unstable_num == m.opt.N
    assert m.get_curr_frame == m.optimize_frames_ids[-1] and m.get_total_iter == m.iter + m.time * args.gaussian_update_iter
    m.update_poses(None)                                                  # no back end: nothing moves (tracker.py:69-74)
    frames = {f.uid: f for f in list(m.processed_frames) + list(m.keyframe_list)}
    before = {u: (f.pose_version, f.c2w.clone()) for u, f in frames.items()}
    new = {u: f.c2w.numpy().copy() for u, f in frames.items()}
    moved = sorted(frames)[-1]
    new[moved][:3, 3] += 0.01
    m.update_poses(new)
    for u, f in frames.items():
        assert f.pose_version > before[u][0]               # a keyframe still in the window is visited twice, as in the reference
        assert torch.allclose(f.c2w, torch.as_tensor(new[u]))
    assert abs(float(frames[moved].c2w[0, 3] - before[moved][1][0, 3]) - 0.01) < 1e-12
    # release: confidence 0 and a new tick for the masked stable rows, nothing moves
    nf = m.opt.n_frozen
    assert nf > 4
    mask = torch.zeros(nf, dtype=torch.bool)
    mask[1] = mask[3] = True
    P = m.opt.params[:m.opt.N].clone()
    m.time = 9
    m.gaussians_release(mask)
    assert torch.equal(m.opt.params[:m.opt.N], P)
    assert float(m.opt.aux["confidence"][1, 0]) == 0 and float(m.opt.aux["confidence"][3, 0]) == 0
    assert int(m.opt.aux["add_tick"][1, 0]) == 9 and int(m.opt.aux["add_tick"][0, 0]) != 9


@pytest.mark.parametrize("leaf,build", [("replica_base.yaml", "replica_args"), ("tum_base.yaml", "tum_args"),
                                        ("scannetpp_base.yaml", "scannetpp_args")])
def test_argument_sets_are_the_references_config_files(leaf, build):
    """replica_args() / tum_args() against configs/base.yaml overlaid with the dataset's base file (the `parent:` chain the
    reference's loader follows): every value the two have in common is equal, and
    every name Mapping / Tracker / Renderer / IcpTracker read from `args` is in the argument set.  The reference's files,
    merged along that chain, are tests/golden/reference_configs.json (oracle/gen_config_golden.py)."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as f:
        ref = json.load(f)[leaf]
    mine = vars(getattr(mp, build)())
    common = sorted(set(ref) & set(mine))
    assert len(common) >= 45, common
    for k in common:
        a, b = ref[k], mine[k]
        if isinstance(a, (list, tuple)):
            assert [float(x) for x in a] == [float(x) for x in b], k
        elif isinstance(a, (bool, str)):
            assert a == b, (k, a, b)
        else:
            assert float(a) == float(b), (k, a, b)
    # what the ported classes read and the files define must all be there
    needed = {"uniform_sample_num", "stable_confidence_thres", "unstable_time_window", "memory_length", "gaussian_update_iter",
              "gaussian_update_frame", "position_lr", "feature_lr", "opacity_lr", "scaling_lr", "rotation_lr", "final_global_iter",
              "feature_lr_coef", "scaling_lr_coef", "rotation_lr_coef", "keyframe_trans_thes", "keyframe_theta_thes",
              "add_depth_thres", "add_color_thres", "add_transmission_thres", "transmission_sample_ratio", "error_sample_ratio",
              "history_merge_max_weight", "renderer_opaque_threshold", "renderer_normal_threshold", "renderer_depth_threshold",
              "color_sigma", "icp_downscales", "icp_downscale_iters", "icp_damping", "icp_distance_threshold",
              "icp_normal_threshold", "icp_sample_distance_threshold", "icp_sample_normal_threshold", "icp_fail_threshold",
              "min_depth", "max_depth", "invalid_confidence_thresh", "global_keyframe_num", "color_weight", "depth_weight",
              "ssim_weight", "normal_weight", "init_opacity", "xyz_factor", "max_radius", "min_radius", "scale_factor"}
    assert needed <= set(common), sorted(needed - set(common))


def test_initial_rotation_follows_the_references_cross_product_rule():
    """SLAM/utils.py:216-221 calls torch.cross WITHOUT a dim; the legacy rule takes the first dimension of size 3, which for a
    sampling pass of exactly THREE points is the batch dimension.  compute_rot keeps that (the maps of the two lifecycles
    differ otherwise: found by oracle/fuzz_mapping_vs_reference.py) - checked here against the legacy call itself."""
    import warnings
    g = torch.Generator().manual_seed(5)
    for n in (1, 2, 3, 4, 7):
        nrm = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
        z = torch.zeros_like(nrm)
        z[:, 2] = 1.0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            axis = torch.cross(z, nrm)                                    # the reference's call, legacy default dim
        axis = axis / (torch.norm(axis, p=2, dim=-1, keepdim=True) + 1e-8)
        angle = torch.acos(torch.sum(z * nrm, dim=1)).unsqueeze(-1)
        want = torch.cat([torch.cos(angle / 2), axis * torch.sin(angle / 2)], dim=1)   # quaternion_from_axis_angle
        got = mp.compute_rot(nrm)
        assert torch.allclose(got, want, atol=1e-6), n
    three = torch.nn.functional.normalize(torch.tensor([[0.1, 0.2, -1.0], [0.3, -0.1, -1.0], [-0.2, 0.1, -1.0]]), dim=1)
    q = mp.compute_rot(three)
    assert float(q[:, 1:3].abs().max()) < 1e-6 and float(q[:, 3].abs().max()) > 0.9      # turned about z (if at all): the quirk
