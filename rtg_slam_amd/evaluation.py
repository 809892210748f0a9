"""Map-quality evaluation of the reference (SLAM/eval.py, metric.py) on the HIP kernels of include/rtgs_slam.h, "evaluation":

    eval_picture       SLAM/eval.py:38-147    PSNR (mean of the per-channel PSNR, utils/loss_utils.py:23-25), MS-SSIM
                                              (pytorch_msssim.ms_ssim, data_range 1), colour L1, depth L1, valid-pixel ratio;
                                              LPIPS is not computed (no pretrained AlexNet weights): None
    eval_pcd           SLAM/eval.py:149-223   accuracy / completion (cm), precision / recall (%) and F1 per threshold, from
                                              the exact 3-NN search (rtgs_knn3_build_ref / _query_built, column 0) and one
                                              reduction kernel per direction
    eval_frame         SLAM/eval.py:225-270   render the map at a frame (under no_grad), then the two above
    evaluate_sequence  metric.py:137-219      every frame of a finished run with the evaluation renderer, the reconstruction
                                              once, per-frame rows and the mean row
    eval_mesh          (no counterpart)       eval_pcd of points sampled on a triangle mesh's surface (rtg_slam_amd.meshing)
    eval_mesh_surface  (no counterpart)       the same keys from samples of each mesh to the other's SURFACE (exact point-to-
                                              triangle distances, mesh_ops.MeshDistance), and the normal consistency
    align_to_gt        (no counterpart)       the rigid transform that registers a reconstruction to the GT surface
                                              (mesh_ops.register_to_mesh), to score shape apart from drift
    VisibilityCull     (no counterpart)       the part of the GT mesh the evaluated frames saw: per vertex, against the sensor
                                              depth, at the GT poses (include/rtgs_slam.h, "visibility")
    MeshRenderer       (no counterpart)       the depth and face maps of a triangle mesh at a pose (include/rtgs_slam.h, "mesh
                                              render"); mesh_depth_metrics: the depth L1 of such a map; render_color: the
                                              mesh in its vertex colours or its baked atlas, mesh_color_metrics: its PSNR,
                                              MS-SSIM and colour L1 against a frame

Each metric call reads its float64 result vector from the device once; that read is its only synchronisation.  The results
are bitwise reproducible run to run (fixed-order reductions, no float atomics).  There is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .io_formats import metrics_mean_row

# layout of rtgs_eval_picture's result vector (include/rtgs_slam.h)
OUT_PSNR, OUT_COLOR_L1, OUT_DEPTH_L1, OUT_VALID_RATIO, OUT_MS_SSIM, OUT_VALID_COUNT, OUT_MSE, OUT_CS, OUT_SSIM = (
    _lib.CONSTANTS["RTGS_EVAL_OUT_" + n] for n in ("PSNR", "COLOR_L1", "DEPTH_L1", "VALID_RATIO", "MS_SSIM", "VALID_COUNT",
                                                   "MSE", "CS", "SSIM"))    # the last three: [3], [5 levels][3 channels], [5][3]
PICTURE_OUT = _lib.CONSTANTS["RTGS_EVAL_PICTURE_OUT"]
MS_SSIM_MIN_SIDE = _lib.CONSTANTS["RTGS_EVAL_MS_SSIM_MIN_SIDE"]      # pytorch_msssim asserts the smaller side is > 160
MAX_THRESHOLDS = _lib.CONSTANTS["RTGS_EVAL_MAX_THRESHOLDS"]


def _dev(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("rtg_slam_amd.evaluation: tensors must live on a HIP device; this build has no CPU path.")
    return ts[0].device


_p, _stream = _lib.ptr, _lib.stream


def picture_metrics(render: torch.Tensor, gt_color: torch.Tensor, depth: torch.Tensor, gt_depth: torch.Tensor,
                    depth_index: torch.Tensor, min_depth: float, max_depth: float, with_ms_ssim: bool = True) -> torch.Tensor:
    """rtgs_eval_picture -> its float64 result vector [PICTURE_OUT], left on the device (no synchronisation).  render /
    gt_color [3,H,W]; depth, gt_depth, depth_index: H*W values each ([1,H,W], [H,W] or [H,W,1])."""
    H, W = int(render.shape[-2]), int(render.shape[-1])
    if with_ms_ssim and min(H, W) <= MS_SSIM_MIN_SIDE:
        raise ValueError(f"rtg_slam_amd.evaluation: MS-SSIM needs the smaller image side > {MS_SSIM_MIN_SIDE}, got {H}x{W}")
    for name, t, n in (("render", render, 3 * H * W), ("gt_color", gt_color, 3 * H * W), ("depth", depth, H * W),
                       ("gt_depth", gt_depth, H * W), ("depth_index", depth_index, H * W)):
        if t.numel() != n:
            raise ValueError(f"rtg_slam_amd.evaluation: {name} has {t.numel()} values, expected {n} for a {H}x{W} image")
    dev = _dev(render, gt_color, depth, gt_depth, depth_index)
    lib = _lib.load()
    r, g = render.detach().float().contiguous(), gt_color.detach().float().contiguous()
    d, gd = depth.detach().float().contiguous(), gt_depth.detach().float().contiguous()
    idx = depth_index.detach().to(torch.int32).contiguous()
    scratch = torch.empty(lib.rtgs_eval_picture_scratch_bytes(H, W), dtype=torch.uint8, device=dev)
    out = torch.empty(PICTURE_OUT, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.rtgs_eval_picture(_p(r), _p(g), _p(d), _p(gd), _p(idx), H, W, float(min_depth), float(max_depth),
                                   int(bool(with_ms_ssim)), _p(scratch), _p(out), _stream(dev))
    _lib.check(rc, "rtgs_eval_picture")
    return out


def eval_picture(render_output: Dict[str, torch.Tensor], gt_color: torch.Tensor, gt_depth: torch.Tensor, min_depth: float,
                 max_depth: float, with_ms_ssim: bool = True) -> Dict:
    """SLAM/eval.py:38-147 on a `Renderer.render` result: gt_color [3,H,W] in 0..1, gt_depth in metres (the reference's
    255 * original_depth).  Keys as the reference's `losses`, plus color_l1 (its l1_loss of the colour, logged there)."""
    v = picture_metrics(render_output["render"], gt_color, render_output["depth"], gt_depth, render_output["depth_index_map"],
                        min_depth, max_depth, with_ms_ssim).cpu().tolist()
    return _picture_result(v, with_ms_ssim)


def _picture_result(v, with_ms_ssim: bool) -> Dict:
    return {
        "valid_pixel_ratio": v[OUT_VALID_RATIO],
        "depth_loss": v[OUT_DEPTH_L1],
        "normal_loss": 0,                                             # eval.py:135: torch.tensor(0)
        "psnr": v[OUT_PSNR],
        "ssim": v[OUT_MS_SSIM] if with_ms_ssim else None,
        "lpips": None,                                                # needs pretrained AlexNet weights: not computed
        "color_l1": v[OUT_COLOR_L1],
    }


# ---- exposure-aware picture metrics: the render brought into the frame's own exposure and white balance before it is scored ----

EXPOSURE_DST_LO, EXPOSURE_DST_HI = 4.0 / 255.0, 251.0 / 255.0        # a clamped frame pixel obeys no affine law
EXPOSURE_ROW_KEYS = ("psnr_ea", "ssim_ea", "color_l1_ea", "gain_r", "gain_g", "gain_b", "offset_r", "offset_g", "offset_b", "code")
EXPOSURE_GATES = ("iters", "huber", "cut", "depth_gate", "t_gate", "var_min", "min_valid")


def exposure_settings(H: int, W: int, **gates) -> Dict:
    """The settings of the exposure-aware fit in force: map_exposure's defaults (its depth gate, its schedule) unless given."""
    from . import map_exposure as me
    unknown = sorted(set(gates) - set(EXPOSURE_GATES))
    if unknown:
        raise ValueError(f"rtg_slam_amd.evaluation: unknown exposure gate(s) {', '.join(unknown)}; known: {', '.join(EXPOSURE_GATES)}")
    g = {k: gates.get(k, me.DEFAULTS["map_exposure_" + k]) for k in EXPOSURE_GATES}
    if g["min_valid"] is None:
        g["min_valid"] = me.min_valid_default(H, W)
    g.update(dst_lo=EXPOSURE_DST_LO, dst_hi=EXPOSURE_DST_HI)
    return g


def _exposure_aware_vector(render_output: Dict[str, torch.Tensor], gt_color: torch.Tensor, gt_depth: torch.Tensor, min_depth: float,
                           max_depth: float, with_ms_ssim: bool = True, **gates) -> torch.Tensor:
    """-> [PICTURE_OUT + RTGS_WHITE_BALANCE_STATE] float64 on the device, no synchronisation: picture_metrics of the corrected render,
    then the state of the fit."""
    from . import map_exposure as me
    render = render_output["render"]
    H, W = int(render.shape[-2]), int(render.shape[-1])
    dev = _dev(render, gt_color, gt_depth)
    g = exposure_settings(H, W, **gates)
    lib = _lib.load()
    maps = [me._f32c(t.detach()) for t in (render, render_output["depth"], gt_color, gt_depth, render_output["T_map"])]
    for t, k in zip(maps, (3, 1, 3, 1, 1)):
        if t.numel() != k * H * W:
            raise ValueError(f"rtg_slam_amd.evaluation: colours must be [3,{H},{W}] and depths / T_map {H * W} values")
    state = me.white_balance_state(dev)                                   # identity: every frame is fitted on its own
    scratch = torch.empty(max(lib.rtgs_white_balance_scratch_bytes(H, W) // 8, 1), dtype=torch.float64, device=dev)
    fit_gates = (g["huber"], g["cut"], g["depth_gate"], g["t_gate"], float("-inf"), float("inf"), g["dst_lo"], g["dst_hi"])
    for k in range(int(g["iters"])):
        me.white_balance_fit(lib, maps, H, W, k, fit_gates, g["var_min"], g["min_valid"], state, scratch, dev)
    chw = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    hwc = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.rtgs_white_balance_apply(_p(maps[0]), H, W, _p(state), _p(chw), _p(hwc), _stream(dev))
    _lib.check(rc, "rtgs_white_balance_apply")
    corrected = torch.where(state[me.WB_FRAME_AT] != 0, maps[0].reshape(3, H, W), chw)      # a refused fit leaves the render alone
    v = picture_metrics(corrected, gt_color, render_output["depth"], gt_depth, render_output["depth_index_map"], min_depth,
                        max_depth, with_ms_ssim)
    return torch.cat([v, state])


def _exposure_aware_result(v, with_ms_ssim: bool) -> Dict:
    from . import map_exposure as me
    st = v[PICTURE_OUT:]
    ab = lambda c, i: st[me.WB_REG * c + i]
    return {"psnr_ea": v[OUT_PSNR], "ssim_ea": v[OUT_MS_SSIM] if with_ms_ssim else None, "color_l1_ea": v[OUT_COLOR_L1],
            "gain_r": ab(1, 0), "gain_g": ab(2, 0), "gain_b": ab(3, 0), "offset_r": ab(1, 1), "offset_g": ab(2, 1),
            "offset_b": ab(3, 1), "code": int(st[me.WB_FRAME_AT])}


def exposure_aware_picture(render_output: Dict[str, torch.Tensor], gt_color: torch.Tensor, gt_depth: torch.Tensor, min_depth: float,
                           max_depth: float, with_ms_ssim: bool = True, **gates) -> Dict:
    """The picture metrics of a `Renderer.render` result after an affine colour correction per channel: a state at identity, the
    four-iteration schedule of rtgs_white_balance_fit with source = the render, target = the frame, T = the render's T_map (the
    depth gate is map_exposure's, the render's channels unbounded, the frame's within 4/255 .. 251/255), rtgs_white_balance_apply
    on the render, picture_metrics of the result.  -> psnr_ea, ssim_ea (MS-SSIM; None without it), color_l1_ea, gain_r/g/b,
    offset_r/g/b and the frame's code; a refused fit (code != 0) leaves the render alone, so the figures are the plain ones.
    gates: iters, huber, cut, depth_gate, t_gate, var_min, min_valid.  One host read."""
    v = _exposure_aware_vector(render_output, gt_color, gt_depth, min_depth, max_depth, with_ms_ssim, **gates).cpu().tolist()
    return _exposure_aware_result(v, with_ms_ssim)


def nn_stats(dist2: torch.Tensor, thresholds: torch.Tensor) -> torch.Tensor:
    """rtgs_eval_nn_stats over column 0 of dist2 [N,3] -> float64 [1 + k] on the device: sum of the distances, then the
    number of distances below each threshold (float64 [k] on the device)."""
    dev = _dev(dist2, thresholds)
    lib = _lib.load()
    d = dist2.detach().float().contiguous()
    N, k = int(d.shape[0]), int(thresholds.numel())
    if d.dim() != 2 or d.shape[1] != 3 or N == 0 or k > MAX_THRESHOLDS:
        raise ValueError(f"rtg_slam_amd.evaluation: dist2 must be [N >= 1, 3] and k <= {MAX_THRESHOLDS}")
    thr = thresholds.to(torch.float64).contiguous()
    scratch = torch.empty(lib.rtgs_eval_nn_stats_scratch_bytes(N, k), dtype=torch.uint8, device=dev)
    out = torch.empty(1 + k, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.rtgs_eval_nn_stats(_p(d), N, _p(thr), k, _p(scratch), _p(out), _stream(dev))
    _lib.check(rc, "rtgs_eval_nn_stats")
    return out


def subsample(points: torch.Tensor, sample_nums: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Rows drawn without replacement down to sample_nums (eval.py:164-165's np.random.choice), or all of them."""
    P = int(points.shape[0])
    if P <= sample_nums:
        return points
    pick = torch.randperm(P, generator=generator)[:int(sample_nums)]
    return points[pick.to(points.device)]


def eval_pcd(rec_points, gt_points, dist_thres: Sequence[float] = (0.03,), transform=None, sample_nums: int = 1_000_000,
             generator: Optional[torch.Generator] = None) -> Dict[str, float]:
    """SLAM/eval.py:149-223 on point sets: rec_points [P,3] (the map's Gaussian centres) on the device, gt_points [M,3]
    (sampled from the GT mesh: io_formats.sample_mesh_surface) as a tensor or array.  `transform` (4x4) moves the
    reconstruction first; it is then subsampled without replacement to sample_nums.  accuracy = mean distance of the
    reconstruction to GT, completion = of GT to the reconstruction, both in cm; P / R = percentage below each threshold;
    F1 = 2PR / (P + R), NaN when P + R = 0."""
    from . import slam_ops as so
    dev = _dev(rec_points)
    rec = rec_points.detach().float().reshape(-1, 3)
    gt = torch.as_tensor(gt_points).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    if rec.shape[0] == 0 or gt.shape[0] == 0:
        raise ValueError("rtg_slam_amd.evaluation: eval_pcd needs non-empty point sets")
    thres = [float(t) for t in dist_thres]
    if len(thres) > MAX_THRESHOLDS:
        raise ValueError(f"rtg_slam_amd.evaluation: at most {MAX_THRESHOLDS} thresholds")
    rec = subsample(rec, sample_nums, generator)
    if transform is not None:
        rec = so.transform_map(rec.contiguous(), torch.as_tensor(np.asarray(transform, dtype=np.float32)))
    rec = rec.contiguous()
    Nr, Ng = int(rec.shape[0]), int(gt.shape[0])
    thr = torch.tensor(thres, dtype=torch.float64, device=dev)
    d_acc, _ = so.knn_query_built(so.knn_build_ref(gt), Ng, rec)        # reconstruction -> GT: accuracy, precision
    d_comp, _ = so.knn_query_built(so.knn_build_ref(rec), Nr, gt)       # GT -> reconstruction: completion, recall
    v = torch.cat([nn_stats(d_acc, thr), nn_stats(d_comp, thr)]).cpu().tolist()
    k = len(thres)
    acc, comp = v[:1 + k], v[1 + k:]
    res = {"accuracy": acc[0] / Nr * 100.0, "completion": comp[0] / Ng * 100.0}
    Ps = {f"P (< {t})": acc[1 + j] / Nr * 100.0 for j, t in enumerate(thres)}
    Rs = {f"R (< {t})": comp[1 + j] / Ng * 100.0 for j, t in enumerate(thres)}
    Fs = {}
    for t in thres:
        P, R = Ps[f"P (< {t})"], Rs[f"R (< {t})"]
        Fs[f"F1 (< {t})"] = 2 * P * R / (P + R) if P + R > 0 else math.nan
    res.update(Ps)
    res.update(Rs)
    res.update(Fs)
    return res


def sample_mesh_points(vertices, faces, n: int, seed: int = 0, device=None) -> torch.Tensor:
    """n points on a mesh's surface (io_formats.sample_mesh_surface: face by area, then uniform inside it; drawn on the host
    in float64) as a float32 [n,3] tensor on `device` (default: the current HIP device)."""
    from .io_formats import sample_mesh_surface
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if device is None:
        device = vertices.device if torch.is_tensor(vertices) and vertices.is_cuda else torch.device("cuda", torch.cuda.current_device())
    pts, _ = sample_mesh_surface(to_np(vertices), to_np(faces), int(n), seed)
    return torch.from_numpy(pts).to(device=device, dtype=torch.float32)


def eval_mesh(vertices, faces, gt_points, dist_thres: Sequence[float] = (0.03,), transform=None, sample_nums: int = 1_000_000,
              seed: int = 0) -> Dict[str, float]:
    """The reconstruction metrics of a triangle mesh: sample_nums points drawn on its surface (sample_mesh_points, `seed`),
    then eval_pcd of them against gt_points; the same keys.  vertices [V,3], faces [F,3]: tensors or arrays."""
    dev = gt_points.device if torch.is_tensor(gt_points) and gt_points.is_cuda else None
    if torch.is_tensor(vertices) and vertices.is_cuda:
        dev = vertices.device
    return eval_pcd(sample_mesh_points(vertices, faces, sample_nums, seed, dev), gt_points, dist_thres, transform, sample_nums)


def _surface_side(samples, own_face, own: "MeshDistance", target: "MeshDistance", thr, max_distance=None):
    """One direction of eval_mesh_surface -> float64 [3 + k] on the device: nn_stats of the samples' distances to the target's
    surface, then the sum of |n_own . n_hit| and the number of samples it runs over.  With max_distance a 4 + k th value
    follows: the rows beyond the bound, whose distance counts as the bound and whose zero normal counts them out."""
    d2, face, n_hit = target.query(samples, normals=True, max_distance=max_distance)
    beyond = None
    if max_distance is not None:
        md = np.float32(max_distance)
        beyond = face < 0
        d2 = torch.where(beyond, torch.full_like(d2, float(md * md)), d2)       # float32 max_d2, as the query formed it
    n_own = own.face_normals(own_face)
    dot = ((n_own[:, 0] * n_hit[:, 0] + n_own[:, 1] * n_hit[:, 1]) + n_own[:, 2] * n_hit[:, 2]).abs()      # float32, step by step
    ok = (n_own != 0).any(1) & (n_hit != 0).any(1)                   # a degenerate face has the normal (0, 0, 0)
    nc = torch.stack([torch.where(ok, dot, torch.zeros_like(dot)).sum(dtype=torch.float64), ok.sum().to(torch.float64)])
    out = [nn_stats(d2[:, None].expand(-1, 3), thr), nc]
    if beyond is not None:
        out.append(beyond.sum().to(torch.float64).reshape(1))
    return torch.cat(out)


def eval_mesh_surface(rec_vertices, rec_faces, gt_vertices, gt_faces, dist_thres: Sequence[float] = (0.03,), transform=None,
                      sample_nums: int = 1_000_000, seed: int = 0, device=None, reports: Optional[Dict] = None,
                      max_distance: Optional[float] = None) -> Dict[str, float]:
    """The reconstruction metrics of a triangle mesh against a GT mesh with the SURFACE on the far side of every distance
    (mesh_ops.MeshDistance), so that no figure carries the sample spacing of the other mesh: accuracy and precision from
    sample_nums points drawn on the reconstruction (sample_mesh_surface, `seed`, as eval_mesh draws them; moved by `transform`
    as eval_pcd moves them) to the GT surface, completion and recall from sample_nums points drawn on the GT mesh (`seed`) to
    the reconstruction's surface (its vertices moved by `transform`).  The keys of eval_pcd, and
        normal_consistency_acc / _comp   the mean |n_sample_face . n_hit_face| of each direction: float32 unit normals, the
                                         absolute value because GT meshes are not all wound towards free space, the sum in
                                         float64; samples whose own or hit face has no area are counted out
        normal_samples_acc / _comp       the samples they run over
        normal_consistency               the mean of the two.
    max_distance = D (metres, > every threshold; a ValueError otherwise) truncates: both directions ask only for the nearest face
    within D (MeshDistance.query(max_distance=D): bounded time against an un-culled GT), a distance beyond D counts as D in
    accuracy and completion, and the normal consistency runs over the samples within D.  P, R and F1 are exactly those of the
    call without it.  The result then also holds max_distance, beyond_acc and beyond_comp, the samples beyond the bound.
    Meshes are arrays or device tensors.  `reports`, a dict, receives "gt" and "rec": the two MeshDistance.report()s."""
    from . import mesh_ops, slam_ops as so
    from .io_formats import sample_mesh_surface
    if device is None:
        device = next((t.device for t in (rec_vertices, rec_faces, gt_vertices, gt_faces) if torch.is_tensor(t) and t.is_cuda), None)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    dev = torch.device(device)
    thres = [float(t) for t in dist_thres]
    if len(thres) > MAX_THRESHOLDS:
        raise ValueError(f"rtg_slam_amd.evaluation: at most {MAX_THRESHOLDS} thresholds")
    if max_distance is not None and not (thres and float(max_distance) > max(thres) and math.isfinite(float(max_distance))):
        raise ValueError(f"rtg_slam_amd.evaluation: max_distance must be finite and above every threshold {thres}, got {max_distance}")
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(to_np(a))).to(device=dev, dtype=dt).contiguous()
    sides = {}
    for name, v, f in (("rec", rec_vertices, rec_faces), ("gt", gt_vertices, gt_faces)):
        pts, own = sample_mesh_surface(to_np(v), to_np(f), int(sample_nums), seed)
        pts, vt = up(pts, torch.float32), up(v, torch.float32).reshape(-1, 3)
        if name == "rec" and transform is not None:
            m = torch.as_tensor(np.asarray(transform, dtype=np.float32))
            pts, vt = so.transform_map(pts, m).contiguous(), so.transform_map(vt, m).contiguous()
        sides[name] = (pts, up(own, torch.int32), mesh_ops.MeshDistance(vt, up(f, torch.int64).reshape(-1, 3).to(torch.int32)))
    thr = torch.tensor(thres, dtype=torch.float64, device=dev)
    (rp, ro, rmd), (gp, go, gmd) = sides["rec"], sides["gt"]
    k = len(thres)
    w = 3 + k + (max_distance is not None)
    v = torch.cat([_surface_side(rp, ro, rmd, gmd, thr, max_distance),
                   _surface_side(gp, go, gmd, rmd, thr, max_distance)]).cpu().tolist()                         # the one host read
    acc, comp = v[:w], v[w:]
    Nr, Ng = int(rp.shape[0]), int(gp.shape[0])
    res = {"accuracy": acc[0] / Nr * 100.0, "completion": comp[0] / Ng * 100.0}
    Ps = {f"P (< {t})": acc[1 + j] / Nr * 100.0 for j, t in enumerate(thres)}
    Rs = {f"R (< {t})": comp[1 + j] / Ng * 100.0 for j, t in enumerate(thres)}
    Fs = {}
    for t in thres:
        P, R = Ps[f"P (< {t})"], Rs[f"R (< {t})"]
        Fs[f"F1 (< {t})"] = 2 * P * R / (P + R) if P + R > 0 else math.nan
    res.update(Ps)
    res.update(Rs)
    res.update(Fs)
    for name, s in (("acc", acc), ("comp", comp)):
        res["normal_consistency_" + name] = s[1 + k] / s[2 + k] if s[2 + k] else math.nan
        res["normal_samples_" + name] = int(s[2 + k])
    res["normal_consistency"] = 0.5 * (res["normal_consistency_acc"] + res["normal_consistency_comp"])
    if max_distance is not None:
        res.update(max_distance=float(max_distance), beyond_acc=int(acc[3 + k]), beyond_comp=int(comp[3 + k]))
    if reports is not None:
        reports["gt"], reports["rec"] = gmd.report(), rmd.report()
    return res


def align_to_gt(rec_points, gt_vertices, gt_faces, transform=None, sample_nums: int = 1_000_000,
                generator: Optional[torch.Generator] = None, source_normals=None, reports: Optional[Dict] = None, **kw):
    """Register a reconstruction rigidly to the GT SURFACE (mesh_ops.register_to_mesh: point-to-plane ICP on exact nearest
    faces) -> (T_total [4,4] float64, report), T_total = T_align @ transform: what eval_pcd and eval_mesh_surface take as
    `transform` to score the aligned reconstruction.  rec_points [P,3] on the device are subsampled without replacement to
    sample_nums as eval_pcd subsamples them (source_normals [P,3], the points' own unit normals, follow the draw), moved by
    `transform` (4x4; the normals by its rotation) and registered from the identity; T_align is the rigid error the
    registration found, the report is register_to_mesh's.  gt_vertices / gt_faces: arrays or device tensors.  **kw goes to
    register_to_mesh (max_distance, max_iterations, min_cos, rank_tol, bounded_query).  `reports`, a dict, receives "gt": the GT's
    MeshDistance.report()."""
    from . import mesh_ops, slam_ops as so
    dev = _dev(rec_points)
    rec = rec_points.detach().float().reshape(-1, 3)
    nrm = None
    if source_normals is not None:
        _dev(source_normals)
        nrm = source_normals.detach().float().reshape(-1, 3)
        if nrm.shape != rec.shape:
            raise ValueError("rtg_slam_amd.evaluation: source_normals must hold one row per point")
    if rec.shape[0] == 0:
        raise ValueError("rtg_slam_amd.evaluation: align_to_gt needs a non-empty point set")
    P = int(rec.shape[0])
    if P > sample_nums:                                                # subsample()'s draw, shared by the points and the normals
        pick = torch.randperm(P, generator=generator)[:int(sample_nums)].to(dev)
        rec, nrm = rec[pick], None if nrm is None else nrm[pick]
    base = np.eye(4) if transform is None else np.asarray(transform, dtype=np.float64).reshape(4, 4)
    if transform is not None:
        m = np.asarray(transform, dtype=np.float32).reshape(4, 4)
        rec = so.transform_map(rec.contiguous(), torch.as_tensor(m))
        if nrm is not None:
            r = m.copy()
            r[:3, 3] = 0.0
            nrm = so.transform_map(nrm.contiguous(), torch.as_tensor(r))
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(to_np(a))).to(device=dev, dtype=dt).contiguous()
    md = mesh_ops.MeshDistance(up(gt_vertices, torch.float32).reshape(-1, 3), up(gt_faces, torch.int64).reshape(-1, 3).to(torch.int32))
    T, report = mesh_ops.register_to_mesh(rec.contiguous(), md, source_normals=None if nrm is None else nrm.contiguous(), **kw)
    if reports is not None:
        reports["gt"] = md.report()
    return T @ base, report


# ---------------------------------------------------------------------------------------------------------------------
# visibility culling of the GT mesh
# ---------------------------------------------------------------------------------------------------------------------

def visibility_add(views: torch.Tensor, points: torch.Tensor, depth: torch.Tensor, K, w2c, tolerance: float) -> None:
    """rtgs_visibility_add: views [N] int32 += 1, in place, for every point of points [N,3] float32 that the frame sees -
    include/rtgs_slam.h, "visibility", steps 1-8.  depth [H,W] or [H,W,1] float32 metres; K = (fx, fy, cx, cy); w2c: the
    world-to-camera matrix (4x4 or its top 3x4), cast to float32 here.  All tensors on one device and contiguous."""
    dev = _dev(views, points, depth)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("rtg_slam_amd.evaluation: points must be [N,3] float32")
    if depth.dim() == 3 and depth.shape[2] == 1:
        depth = depth[:, :, 0] if depth.is_contiguous() else depth       # [H,W,1] contiguous is [H,W] contiguous
    if depth.dim() != 2 or depth.dtype != torch.float32 or depth.numel() == 0:
        raise ValueError("rtg_slam_amd.evaluation: depth must be a non-empty [H,W] or [H,W,1] float32 image")
    N = int(points.shape[0])
    if views.shape != (N,) or views.dtype != torch.int32:
        raise ValueError("rtg_slam_amd.evaluation: views must be [N] int32, one count per point")
    if not (points.is_contiguous() and depth.is_contiguous() and views.is_contiguous()):
        raise ValueError("rtg_slam_amd.evaluation: points, depth and views must be contiguous")
    if points.device != dev or depth.device != dev:
        raise ValueError("rtg_slam_amd.evaluation: points, depth and views live on different devices")
    tolerance = float(np.float32(tolerance))
    if not tolerance >= 0:
        raise ValueError(f"rtg_slam_amd.evaluation: the visibility tolerance must be >= 0, got {tolerance}")
    m = np.ascontiguousarray(np.asarray(w2c, dtype=np.float32).reshape(-1)[:12])
    if m.size != 12:
        raise ValueError("rtg_slam_amd.evaluation: w2c must be a 4x4 or 3x4 matrix")
    H, W = int(depth.shape[0]), int(depth.shape[1])
    fx, fy, cx, cy = (float(np.float32(k)) for k in K)
    with torch.cuda.device(dev):
        rc = _lib.load().rtgs_visibility_add(_p(points), N, _p(depth), H, W, fx, fy, cx, cy, (C.c_float * 12)(*m.tolist()),
                                             tolerance, _p(views), _stream(dev))
    _lib.check(rc, "rtgs_visibility_add")


def visibility_keep_faces(faces: torch.Tensor, views: torch.Tensor, min_views: int = 1, any_vertex: bool = False) -> torch.Tensor:
    """rtgs_visibility_keep_faces -> keep [F] int32: 1 where all three corners of faces [F,3] int32 (any_vertex: at least one)
    have views >= min_views.  The face indices are checked against len(views) here (one host synchronisation)."""
    dev = _dev(faces, views)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError("rtg_slam_amd.evaluation: faces must be [F,3] int32")
    if views.dim() != 1 or views.dtype != torch.int32 or views.device != dev:
        raise ValueError("rtg_slam_amd.evaluation: views must be [V] int32 on the faces' device")
    if not (faces.is_contiguous() and views.is_contiguous()):
        raise ValueError("rtg_slam_amd.evaluation: faces and views must be contiguous")
    min_views = int(min_views)
    if not -2 ** 31 <= min_views < 2 ** 31:
        raise ValueError("rtg_slam_amd.evaluation: min_views must fit int32")
    F, V = int(faces.shape[0]), int(views.shape[0])
    if F:
        lo, hi = (int(x) for x in torch.aminmax(faces))
        if lo < 0 or hi >= V:
            raise ValueError(f"rtg_slam_amd.evaluation: face indices must lie in 0..{V - 1}, found {lo}..{hi}")
    keep = torch.empty(F, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().rtgs_visibility_keep_faces(_p(faces), F, _p(views), min_views, int(bool(any_vertex)), _p(keep),
                                                    _stream(dev))
    _lib.check(rc, "rtgs_visibility_keep_faces")
    return keep


class VisibilityCull:
    """The part of a GT mesh that a sequence of frames saw.  A vertex is seen by a frame when it projects, at the frame's GT
    pose, into a pixel whose SENSOR depth is valid and not more than `tolerance` metres in front of it (visibility_add); a face
    stays when all of its corners (keep "any": at least one) were seen by min_views frames or more.

        cull = VisibilityCull(vertices, faces, cam, transform=pose_t0)
        for depth, _, gt_c2w in stream: cull.add(depth, gt_c2w)
        v, f = cull.mesh()

    vertices [V,3] and faces [F,3] are arrays or device tensors; they are cast to float32 / int32 once, here.  `transform` is
    the 4x4 evaluate_sequence receives (datasets.read_pose_t0): the stream's poses are relative to the first frame, transform @
    c2w is the camera in the mesh's frame.  The default tolerance is the F-score threshold of metric (dist_thres = [0.03])."""

    def __init__(self, vertices, faces, cam, transform=None, tolerance: float = 0.03, min_views: int = 1, any_vertex: bool = False,
                 device=None):
        for t in (vertices, faces):
            if torch.is_tensor(t) and not t.is_cuda:
                raise RuntimeError("rtg_slam_amd.evaluation: tensors must live on a HIP device; this build has no CPU path.")
        if device is None:
            device = next((t.device for t in (vertices, faces) if torch.is_tensor(t)), None)
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("rtg_slam_amd.evaluation: VisibilityCull needs a HIP device; this build has no CPU path.")
        V = int(vertices.shape[0])
        if V >= 2 ** 31:
            raise ValueError(f"rtg_slam_amd.evaluation: {V} vertices do not fit the int32 face indices")
        up = lambda a, dt: (a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=self.device, dtype=dt)
        self.vertices = up(vertices, torch.float32).reshape(-1, 3).contiguous()
        f = up(faces, torch.int64).reshape(-1, 3)
        if f.shape[0]:
            lo, hi = (int(x) for x in torch.aminmax(f))
            if lo < 0 or hi >= V:
                raise ValueError(f"rtg_slam_amd.evaluation: face indices must lie in 0..{V - 1}, found {lo}..{hi}")
        self.faces = f.to(torch.int32).contiguous()
        self.cam = cam
        self.transform = np.eye(4) if transform is None else np.asarray(transform, dtype=np.float64).reshape(4, 4)
        self.tolerance = float(np.float32(tolerance))
        self.min_views = int(min_views)
        self.any_vertex = bool(any_vertex)
        if not self.tolerance >= 0:
            raise ValueError(f"rtg_slam_amd.evaluation: the visibility tolerance must be >= 0, got {tolerance}")
        if self.min_views < 1:
            raise ValueError(f"rtg_slam_amd.evaluation: min_views must be >= 1, got {min_views}")
        self.views = torch.zeros(V, dtype=torch.int32, device=self.device)
        self.frames = 0
        self._events: List = []
        self._seconds = 0.0

    def add(self, depth: torch.Tensor, c2w) -> None:
        """One frame: depth [H,W] or [H,W,1] float32 on the device, at the camera's size; c2w its GT pose as the stream gives
        it.  The matrix used is inv(transform @ c2w), inverted in float64 on the host, then cast to float32."""
        if not torch.is_tensor(depth) or not depth.is_cuda:
            raise RuntimeError("rtg_slam_amd.evaluation: tensors must live on a HIP device; this build has no CPU path.")
        if tuple(depth.shape[:2]) != (self.cam.H, self.cam.W):
            raise ValueError(f"rtg_slam_amd.evaluation: depth is {tuple(depth.shape)}, the camera {self.cam.H}x{self.cam.W}")
        c2w = c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else np.asarray(c2w)
        w2c = np.linalg.inv(self.transform @ c2w.astype(np.float64).reshape(4, 4)).astype(np.float32)
        with torch.cuda.device(self.device):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            visibility_add(self.views, self.vertices, depth, (self.cam.fx, self.cam.fy, self.cam.cx, self.cam.cy), w2c, self.tolerance)
            b.record()
        self._events.append((a, b))
        self.frames += 1

    def keep(self) -> torch.Tensor:
        """-> keep [F] int32 for the frames added so far."""
        return visibility_keep_faces(self.faces, self.views, self.min_views, self.any_vertex)

    def mesh(self):
        """-> (vertices [V_kept,3] float32, faces [F_kept,3] int32) on the device: the kept faces in their order, the vertices
        they use in theirs, faces re-indexed (mesh_ops.keep_faces)."""
        from . import mesh_ops
        v, f, _ = mesh_ops.keep_faces(self.vertices, self.faces, None, self.keep())
        return v, f

    def report(self) -> Dict:
        """Counts before and after, the settings, and the device time of the .add launches (events; synchronises)."""
        for a, b in self._events:
            b.synchronize()
            self._seconds += a.elapsed_time(b) * 1e-3
        self._events = []
        v, f = self.mesh()
        return {"V": int(self.vertices.shape[0]), "F": int(self.faces.shape[0]), "V_kept": int(v.shape[0]), "F_kept": int(f.shape[0]),
                "frames": self.frames, "tolerance": self.tolerance, "min_views": self.min_views,
                "keep": "any" if self.any_vertex else "all", "seconds": self._seconds}


# ---------------------------------------------------------------------------------------------------------------------
# rendering a triangle mesh: depth and face maps
# ---------------------------------------------------------------------------------------------------------------------

MESH_RENDER_NEAR = 0.05
# Boxes of more than this many pixels go to the wave path of csrc/mesh_render.hip (DESIGN.md §4h has the measurement).
MESH_RENDER_SMALL_MAX = 16
MESH_TEXTURE_MAX_SIDE = _lib.CONSTANTS["RTGS_MESH_TEXTURE_MAX_SIDE"]


class MeshRenderer:
    """The depth map and the face map of a triangle mesh at a pinhole pose (include/rtgs_slam.h, "mesh render"): per pixel
    centre the nearest surface and the face it belongs to, both windings, bit for bit tests/mesh_render_reference.py.

        r = MeshRenderer(vertices, faces, cam, transform=pose_t0)
        depth, face = r.render(c2w)            # [H,W] float32 metres (0: nothing), [H,W] int32 (-1: nothing)

    vertices [V,3] and faces [F,3] are arrays or device tensors, cast to float32 / int32 and checked once, here, as
    VisibilityCull does; `transform @ c2w` is the camera in the mesh's frame.  A face with a corner at or behind `near` metres
    is dropped whole, not clipped: a camera within `near` of a large triangle sees a hole there.  small_max: the largest pixel
    box one thread walks (larger faces take a wave each); it changes the time only, never the picture.

        r = MeshRenderer(vertices, faces, cam, colors=colors, uv=uv, texture=image)
        color, depth, face = r.render_color(c2w, source="texture")        # [3,H,W] float32 in 0..1

    colors [V,3] float32 in 0..1, uv [F,3,2] float32 (y down, as meshing.texture_mesh and load_textured_obj give it) and
    texture [Ht,Wt,3] uint8 are the colour sources of render_color, cast and checked once, here; without them the object and
    render() are what they are."""

    def __init__(self, vertices, faces, cam, transform=None, near: float = MESH_RENDER_NEAR, small_max: Optional[int] = None,
                 device=None, colors=None, uv=None, texture=None):
        for t in (vertices, faces):
            if torch.is_tensor(t) and not t.is_cuda:
                raise RuntimeError("rtg_slam_amd.evaluation: tensors must live on a HIP device; this build has no CPU path.")
        if device is None:
            device = next((t.device for t in (vertices, faces) if torch.is_tensor(t)), None)
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("rtg_slam_amd.evaluation: MeshRenderer needs a HIP device; this build has no CPU path.")
        self.near = float(np.float32(near))
        if not self.near > 0:
            raise ValueError(f"rtg_slam_amd.evaluation: near must be > 0, got {near}")
        self.small_max = MESH_RENDER_SMALL_MAX if small_max is None else int(small_max)
        if not 0 <= self.small_max < 2 ** 31:
            raise ValueError(f"rtg_slam_amd.evaluation: small_max must lie in 0..2^31 - 1, got {small_max}")
        V = int(vertices.shape[0])
        if V >= 2 ** 31:
            raise ValueError(f"rtg_slam_amd.evaluation: {V} vertices do not fit the int32 face indices")
        up = lambda a, dt: (a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=self.device, dtype=dt)
        self.vertices = up(vertices, torch.float32).reshape(-1, 3).contiguous()
        f = up(faces, torch.int64).reshape(-1, 3)
        if f.shape[0] >= 2 ** 31:
            raise ValueError(f"rtg_slam_amd.evaluation: {f.shape[0]} faces do not fit the int32 face map")
        if f.shape[0]:
            lo, hi = (int(x) for x in torch.aminmax(f))
            if lo < 0 or hi >= V:
                raise ValueError(f"rtg_slam_amd.evaluation: face indices must lie in 0..{V - 1}, found {lo}..{hi}")
        self.faces = f.to(torch.int32).contiguous()
        self.cam = cam
        H, W = int(cam.H), int(cam.W)
        if H <= 0 or W <= 0 or H * W >= 2 ** 31:
            raise ValueError(f"rtg_slam_amd.evaluation: cannot render a {H}x{W} picture")
        self.transform = np.eye(4) if transform is None else np.asarray(transform, dtype=np.float64).reshape(4, 4)
        n = _lib.load().rtgs_mesh_render_scratch_bytes(V, int(self.faces.shape[0]), H, W)
        self._scratch = torch.empty((n + 7) // 8, dtype=torch.int64, device=self.device)      # once; 8-byte aligned keys
        self.colors, self.uv, self.texture = self._color_sources(colors, uv, texture, V, int(self.faces.shape[0]))
        self.renders = 0
        self._events: List = []
        self._seconds = 0.0

    def _color_sources(self, colors, uv, texture, V: int, F: int):
        """The colour sources, cast and checked once -> (colors [V,3] float32, uv [F,3,2] float32, texture [Ht,Wt,3] uint8) on
        the device, None for what was not given."""
        def up(name, a, shape, dtypes, dt):
            if torch.is_tensor(a) and not a.is_cuda:
                raise RuntimeError("rtg_slam_amd.evaluation: tensors must live on a HIP device; this build has no CPU path.")
            t = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
            if t.dtype not in dtypes:
                raise ValueError(f"rtg_slam_amd.evaluation: {name} must be {dtypes[0]}, got {t.dtype}")
            if t.dim() != len(shape) or any(want is not None and int(got) != want for got, want in zip(t.shape, shape)):
                want = "[" + ",".join("*" if k is None else str(k) for k in shape) + "]"
                raise ValueError(f"rtg_slam_amd.evaluation: {name} must have the shape {want}, got {tuple(t.shape)}")
            return t.to(device=self.device, dtype=dt).contiguous()
        floats = (torch.float32, torch.float64)
        if colors is not None:
            colors = up("colors", colors, (V, 3), floats, torch.float32)
        if (uv is None) != (texture is None):
            raise ValueError(f"rtg_slam_amd.evaluation: {'texture' if uv is None else 'uv'} needs "
                             f"{'uv' if uv is None else 'texture'} beside it")
        if uv is not None:
            uv = up("uv", uv, (F, 3, 2), floats, torch.float32)
            texture = up("texture", texture, (None, None, 3), (torch.uint8,), torch.uint8)
            Ht, Wt = int(texture.shape[0]), int(texture.shape[1])
            if not (1 <= Ht <= MESH_TEXTURE_MAX_SIDE and 1 <= Wt <= MESH_TEXTURE_MAX_SIDE):
                raise ValueError(f"rtg_slam_amd.evaluation: texture must be 1..{MESH_TEXTURE_MAX_SIDE} texels on a side, got {Ht}x{Wt}")
        return colors, uv, texture

    def _view(self, c2w):
        """-> the 12 floats of inv(transform @ c2w) (inverted in float64 on the host, then cast to float32), H, W, fx .. cy."""
        c2w = c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else np.asarray(c2w)
        if c2w.size != 16:
            raise ValueError(f"rtg_slam_amd.evaluation: c2w must be a 4x4 matrix, got shape {tuple(c2w.shape)}")
        w2c = np.linalg.inv(self.transform @ c2w.astype(np.float64).reshape(4, 4)).astype(np.float32)
        m = np.ascontiguousarray(w2c.reshape(-1)[:12])
        fx, fy, cx, cy = (float(np.float32(k)) for k in (self.cam.fx, self.cam.fy, self.cam.cx, self.cam.cy))
        return (C.c_float * 12)(*m.tolist()), int(self.cam.H), int(self.cam.W), fx, fy, cx, cy

    def render_color(self, c2w, source: str = "vertex", background=(0.0, 0.0, 0.0)):
        """-> (color [3,H,W] float32, depth [H,W] float32, face [H,W] int32), new tensors: render()'s maps, then the colour pass
        (rtgs_mesh_shade) with the same float32 matrix, bit for bit tests/mesh_shade_reference.py.  source "vertex": the
        perspective-correct blend of the face's three `colors`, clamped to 0..1; "texture": `texture` sampled bilinearly at the
        blend of the face's three `uv` (y down).  A pixel no face covers gets `background`.  No anti-aliasing, no mip levels, no
        lighting.  No synchronisation."""
        if source not in ("vertex", "texture"):
            raise ValueError(f"rtg_slam_amd.evaluation: source must be 'vertex' or 'texture', got {source!r}")
        if source == "vertex" and self.colors is None:
            raise ValueError("rtg_slam_amd.evaluation: source 'vertex' needs the renderer built with colors")
        if source == "texture" and self.uv is None:
            raise ValueError("rtg_slam_amd.evaluation: source 'texture' needs the renderer built with uv and texture")
        bg = np.asarray(background, dtype=np.float32).reshape(-1)
        if bg.size != 3:
            raise ValueError(f"rtg_slam_amd.evaluation: background must hold 3 values, got {bg.size}")
        m, H, W, fx, fy, cx, cy = self._view(c2w)
        V, F = int(self.vertices.shape[0]), int(self.faces.shape[0])
        depth = torch.empty(H, W, dtype=torch.float32, device=self.device)
        face = torch.empty(H, W, dtype=torch.int32, device=self.device)
        color = torch.empty(3, H, W, dtype=torch.float32, device=self.device)
        # an empty tensor has no address: a source of no rows is still named by a pointer the kernel never follows
        named = lambda t: _p(t) if t.numel() else _p(self._scratch)
        null = C.c_void_p(None)
        vertex = source == "vertex"
        lib = _lib.load()
        with torch.cuda.device(self.device):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = lib.rtgs_mesh_render(_p(self.vertices), V, _p(self.faces), F, H, W, fx, fy, cx, cy, m, self.near, self.small_max,
                                      _p(self._scratch), _p(depth), _p(face), _stream(self.device))
            _lib.check(rc, "rtgs_mesh_render")
            rc = lib.rtgs_mesh_shade(
                _p(self.vertices), V, _p(self.faces), F, _p(face), H, W, fx, fy, cx, cy, m, self.near,
                named(self.colors) if vertex else null, null if vertex else named(self.uv), null if vertex else _p(self.texture),
                1 if vertex else int(self.texture.shape[0]), 1 if vertex else int(self.texture.shape[1]),
                (C.c_float * 3)(*bg.tolist()), _p(color), _stream(self.device))
            b.record()
        _lib.check(rc, "rtgs_mesh_shade")
        self._events.append((a, b))
        self.renders += 1
        return color, depth, face

    def render(self, c2w):
        """-> (depth [H,W] float32, face [H,W] int32), new tensors.  c2w: the camera's pose as the stream gives it; the matrix
        used is inv(transform @ c2w), inverted in float64 on the host, then cast to float32.  No synchronisation."""
        c2w = c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else np.asarray(c2w)
        if c2w.size != 16:
            raise ValueError(f"rtg_slam_amd.evaluation: c2w must be a 4x4 matrix, got shape {tuple(c2w.shape)}")
        w2c = np.linalg.inv(self.transform @ c2w.astype(np.float64).reshape(4, 4)).astype(np.float32)
        m = np.ascontiguousarray(w2c.reshape(-1)[:12])
        H, W = int(self.cam.H), int(self.cam.W)
        fx, fy, cx, cy = (float(np.float32(k)) for k in (self.cam.fx, self.cam.fy, self.cam.cx, self.cam.cy))
        depth = torch.empty(H, W, dtype=torch.float32, device=self.device)
        face = torch.empty(H, W, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = _lib.load().rtgs_mesh_render(_p(self.vertices), int(self.vertices.shape[0]), _p(self.faces), int(self.faces.shape[0]),
                                              H, W, fx, fy, cx, cy, (C.c_float * 12)(*m.tolist()), self.near, self.small_max,
                                              _p(self._scratch), _p(depth), _p(face), _stream(self.device))
            b.record()
        _lib.check(rc, "rtgs_mesh_render")
        self._events.append((a, b))
        self.renders += 1
        return depth, face

    @property
    def seconds(self) -> float:
        """The device time of the renders so far (events, read here: synchronises on the last one)."""
        for a, b in self._events:
            b.synchronize()
            self._seconds += a.elapsed_time(b) * 1e-3
        self._events = []
        return self._seconds


def _mesh_depth_sums(mesh_depth: torch.Tensor, ref_depth: torch.Tensor, min_depth: float, max_depth: float) -> torch.Tensor:
    """-> float64 [2] on the device: the number of valid pixels, the sum of |mesh_depth - ref_depth| over them."""
    dev = _dev(mesh_depth, ref_depth)
    if mesh_depth.dtype != torch.float32 or ref_depth.dtype != torch.float32:
        raise ValueError("rtg_slam_amd.evaluation: mesh_depth and ref_depth must be float32")
    if mesh_depth.numel() == 0 or mesh_depth.numel() != ref_depth.numel() or ref_depth.device != dev:
        raise ValueError(f"rtg_slam_amd.evaluation: mesh_depth {tuple(mesh_depth.shape)} and ref_depth {tuple(ref_depth.shape)} "
                         "must hold the same, non-zero number of pixels on one device")
    m, r = mesh_depth.detach().reshape(-1), ref_depth.detach().reshape(-1)
    lo, hi = float(np.float32(min_depth)), float(np.float32(max_depth))
    valid = (m > 0) & (r > lo) & (r < hi)
    diff = torch.where(valid, (m - r).abs(), torch.zeros_like(m))              # float32 differences, summed in float64
    return torch.stack([valid.sum().to(torch.float64), diff.sum(dtype=torch.float64)])


def _mesh_depth_result(sums, n_pixels: int, suffix: str = "") -> Dict[str, float]:
    n, s = float(sums[0]), float(sums[1])
    return {"mesh_valid_ratio" + suffix: n / n_pixels, "mesh_depth_l1" + suffix: s / n if n else 0.0}


def mesh_depth_metrics(mesh_depth: torch.Tensor, ref_depth: torch.Tensor, min_depth: float, max_depth: float) -> Dict[str, float]:
    """The depth L1 of a rendered mesh against a reference depth (a sensor frame, or a render of the GT mesh), in metres:
    valid pixels are those with mesh_depth > 0 and min_depth < ref_depth < max_depth; "mesh_valid_ratio" is their share,
    "mesh_depth_l1" the float64 mean of the float32 |mesh_depth - ref_depth| over them (0 without any).  One host read."""
    return _mesh_depth_result(_mesh_depth_sums(mesh_depth, ref_depth, min_depth, max_depth).cpu().tolist(), mesh_depth.numel())


def _mesh_color_vector(color: torch.Tensor, gt_color: torch.Tensor, face: torch.Tensor, with_ms_ssim: bool) -> torch.Tensor:
    """-> float64 [PICTURE_OUT + 2] on the device: rtgs_eval_picture's vector of the whole picture, the number of hit pixels
    (face >= 0), the sum of |color - gt_color| over their three channels."""
    dev = _dev(color, gt_color, face)
    if color.dtype != torch.float32 or color.dim() != 3 or color.shape[0] != 3:
        raise ValueError(f"rtg_slam_amd.evaluation: color must be [3,H,W] float32, got {tuple(color.shape)} {color.dtype}")
    H, W = int(color.shape[1]), int(color.shape[2])
    if gt_color.numel() != 3 * H * W or face.numel() != H * W or H * W == 0 or gt_color.device != dev or face.device != dev:
        raise ValueError(f"rtg_slam_amd.evaluation: gt_color {tuple(gt_color.shape)} and face {tuple(face.shape)} do not fit a "
                         f"{H}x{W} picture on one device")
    c, g = color.detach(), gt_color.detach().float().reshape(3, H, W)
    none = torch.zeros(H, W, dtype=torch.float32, device=dev)                  # no depth is scored here
    pic = picture_metrics(c, g, none, none, none.to(torch.int32), 0.0, 1.0, with_ms_ssim)
    hit = face.detach().reshape(1, H, W) >= 0
    diff = torch.where(hit, (c - g).abs(), torch.zeros_like(c))                # float32 differences, summed in float64
    return torch.cat([pic, torch.stack([hit.sum().to(torch.float64), diff.sum(dtype=torch.float64)])])


def _mesh_color_result(v, n_pixels: int, with_ms_ssim: bool, suffix: str = "") -> Dict:
    n, s = float(v[PICTURE_OUT]), float(v[PICTURE_OUT + 1])
    return {"mesh_hit_ratio" + suffix: n / n_pixels, "mesh_psnr" + suffix: v[OUT_PSNR],
            "mesh_ssim" + suffix: v[OUT_MS_SSIM] if with_ms_ssim else None, "mesh_color_l1" + suffix: v[OUT_COLOR_L1],
            "mesh_color_l1_hit" + suffix: s / (3.0 * n) if n else 0.0}


def mesh_color_metrics(color: torch.Tensor, gt_color: torch.Tensor, face: torch.Tensor, with_ms_ssim: bool = True) -> Dict:
    """A colour render of a mesh (MeshRenderer.render_color: color [3,H,W] float32, face [H,W]) against a frame's colour
    [3,H,W] in 0..1.  "mesh_hit_ratio" is the share of pixels with face >= 0.  "mesh_psnr", "mesh_ssim" (MS-SSIM; None without
    with_ms_ssim) and "mesh_color_l1" cover the WHOLE picture as eval_picture scores the map's (rtgs_eval_picture): a hole counts
    as the background it was given, as an un-rendered pixel counts against the map.  "mesh_color_l1_hit" is the float64 mean of
    the float32 |color - gt_color| over the hit pixels' channels only (0 without any).  One host read."""
    v = _mesh_color_vector(color, gt_color, face, with_ms_ssim).cpu().tolist()
    return _mesh_color_result(v, int(face.numel()), with_ms_ssim)


def eval_frame(mapper, frame, gt_color: torch.Tensor, gt_depth: torch.Tensor, min_depth: Optional[float] = None,
               max_depth: Optional[float] = None, renderer=None, run_picture: bool = True, run_pcd: bool = False,
               gt_points=None, dist_thres: Sequence[float] = (0.03,), sample_nums: int = 1_000_000, transform=None,
               generator: Optional[torch.Generator] = None, with_ms_ssim: bool = True, exposure_aware: bool = False,
               exposure_gates: Optional[Dict] = None, exposure_events: Optional[List] = None) -> Dict:
    """SLAM/eval.py:225-270: the map (mapper.global_params) rendered at `frame` under no_grad, then eval_picture; eval_pcd
    on the map's Gaussian centres when run_pcd and gt_points are given.  renderer=None renders with the mapper's own
    renderer, as slam.py does, through Mapping._render: a full render of the same frame, pose and map made just before
    (get_render_output) is reused, not redone.  With exposure_aware the row gains exposure_aware_picture's keys (gates from
    exposure_gates) in the same single host read; exposure_events, a list, receives the pair of HIP events around that stage."""
    a = mapper.args
    min_depth = a.min_depth if min_depth is None else min_depth
    max_depth = a.max_depth if max_depth is None else max_depth
    losses: Dict = {}
    with torch.no_grad():
        if run_picture:
            out = mapper._render(frame, "all") if renderer is None else renderer.render(frame, mapper.global_params)
            if not exposure_aware:
                losses.update(eval_picture(out, gt_color, gt_depth, min_depth, max_depth, with_ms_ssim))
            else:
                plain = picture_metrics(out["render"], gt_color, out["depth"], gt_depth, out["depth_index_map"], min_depth,
                                        max_depth, with_ms_ssim)
                if exposure_events is not None:
                    exposure_events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                    exposure_events[-1][0].record()
                ea = _exposure_aware_vector(out, gt_color, gt_depth, min_depth, max_depth, with_ms_ssim, **(exposure_gates or {}))
                if exposure_events is not None:
                    exposure_events[-1][1].record()
                v = torch.cat([plain, ea]).cpu().tolist()                                    # the one host read
                losses.update(_picture_result(v[:PICTURE_OUT], with_ms_ssim))
                losses.update(_exposure_aware_result(v[PICTURE_OUT:], with_ms_ssim))
        if run_pcd and gt_points is not None:
            losses.update(eval_pcd(mapper.opt.gaussian_data("all")["xyz"], gt_points, dist_thres, transform, sample_nums,
                                   generator))
    return losses


def evaluate_sequence(mapper, cam, stream: Iterable, poses=None, args=None, gt_points=None, dist_thres: Sequence[float] = (0.03,),
                      transform=None, sample_nums: int = 1_000_000, generator: Optional[torch.Generator] = None,
                      with_ms_ssim: bool = True, rec_points: Optional[torch.Tensor] = None,
                      gt_cull: Optional["VisibilityCull"] = None, mesh_renderer: Optional["MeshRenderer"] = None,
                      gt_mesh_renderer: Optional["MeshRenderer"] = None, gt_cull_depth: str = "sensor",
                      mesh_color: Optional[str] = None, mesh_texture_renderer: Optional["MeshRenderer"] = None,
                      mesh_color_hook=None, exposure_aware: bool = False, exposure_gates: Optional[Dict] = None) -> Dict:
    """metric.py:137-219 over a finished map.  `stream` yields (depth [H,W] metres, colour [3,H,W], GT c2w) as run_sequence's
    does; frame i is rendered at poses[i] (the estimated trajectory, e.g. tracker.pose_es) or, without poses, at its GT pose,
    by a Renderer whose opaque threshold is args.renderer_opaque_threshold_eval (metric.py:138).  With gt_points, the
    reconstruction metrics join the last frame's row, as metric.py runs them there: of rec_points [P,3] on the device (the
    points of pcd_densify.ply, metric.py:156-163) when given, else of the map's Gaussian centres.
    With gt_cull (a VisibilityCull of the GT mesh), every frame's sensor depth and GT pose - never the estimated one, so the
    culled GT does not depend on the run being scored - go to gt_cull.add while the stream passes, and the GT points of the
    last frame's row are sampled from the culled mesh: as many as gt_points holds, 1 000 000 without gt_points.
    With gt_cull_depth "mesh" the depth gt_cull.add receives is not the sensor's but gt_mesh_renderer's: the GT mesh's own depth
    at the GT pose, which has no holes and no noise (gt_mesh_renderer is a MeshRenderer of the GT mesh with the cull's transform).
    With mesh_renderer (a MeshRenderer of the reconstructed mesh, in the stream's frame) every frame also renders that mesh at
    the pose the map is rendered at and scores its depth against the sensor depth (mesh_depth_metrics, args.min_depth and
    max_depth) and, with gt_mesh_renderer, against the GT mesh rendered at the GT pose (keys ending in _gt).  These rows are
    returned apart, under "mesh_depth_rows" and "mesh_depth_mean", and read from the device once, after the last frame: "rows"
    and "mean" are what they are without the mesh renderers.
    With mesh_color ("vertex", "texture" or "both"; needs mesh_renderer) the mesh is also rendered in colour at that pose
    (MeshRenderer.render_color, black background) and scored against the frame's colour (mesh_color_metrics): the vertex source
    by mesh_renderer, the texture source - its keys end in _tex - by mesh_texture_renderer when one is given (the textured mesh
    need not be the mesh whose depth is scored), else by mesh_renderer.  These rows come under "mesh_color_rows" and
    "mesh_color_mean", read from the device once, after the last frame; everything else is what it is without mesh_color.
    mesh_color_hook(i, source, color) receives every colour render ([3,H,W] on the device) as it is made.
    With exposure_aware every frame's render is also scored in the frame's own exposure and white balance
    (exposure_aware_picture, gates from exposure_gates), in the frame's one host read.  These rows come apart, under
    "exposure_rows" (frame, psnr, psnr_ea, ssim_ea, color_l1_ea, gain_r/g/b, offset_r/g/b, code) and "exposure_mean" (with
    "frames_refused"), with "exposure_seconds", the device time of the stage; "rows" and "mean" are what they are without it.
    Returns {"rows": one dict per frame (with "frame" and "iter"), "mean": the mean row of metric.py:205-211}."""
    if gt_cull_depth not in ("sensor", "mesh"):
        raise ValueError(f"rtg_slam_amd.evaluation: gt_cull_depth must be 'sensor' or 'mesh', got {gt_cull_depth!r}")
    if gt_cull_depth == "mesh" and (gt_cull is None or gt_mesh_renderer is None):
        raise ValueError("rtg_slam_amd.evaluation: gt_cull_depth='mesh' needs gt_cull and gt_mesh_renderer")
    if mesh_color not in (None, "vertex", "texture", "both"):
        raise ValueError(f"rtg_slam_amd.evaluation: mesh_color must be None, 'vertex', 'texture' or 'both', got {mesh_color!r}")
    if mesh_color is not None and mesh_renderer is None:
        raise ValueError("rtg_slam_amd.evaluation: mesh_color needs mesh_renderer")
    color_sources = [] if mesh_color is None else [s for s in ("vertex", "texture") if mesh_color in (s, "both")]
    color_vectors: List[torch.Tensor] = []
    from .mapping import Frame
    from .render import Renderer
    args = mapper.args if args is None else args
    eval_args = SimpleNamespace(**vars(args))
    eval_args.renderer_opaque_threshold = float(getattr(args, "renderer_opaque_threshold_eval", 0.5))
    renderer = Renderer(eval_args)
    rows: List[Dict] = []
    exposure_rows: List[Dict] = []
    exposure_events: List = []
    mesh_sums: List[torch.Tensor] = []
    for i, (depth, color, gt_c2w) in enumerate(stream):
        frame = Frame(cam, gt_c2w, mapper.device, uid=i)
        gt_mesh_depth = None
        if gt_mesh_renderer is not None and (mesh_renderer is not None or gt_cull_depth == "mesh"):
            gt_mesh_depth, _ = gt_mesh_renderer.render(gt_c2w)
        if gt_cull is not None:
            gt_cull.add(gt_mesh_depth if gt_cull_depth == "mesh" else depth, gt_c2w)
        if poses is not None:
            frame.updatePose(np.asarray(poses[i], dtype=np.float64))         # metric.py:175-176
        if mesh_renderer is not None:
            mesh_depth, _ = mesh_renderer.render(poses[i] if poses is not None else gt_c2w)
            sums = [_mesh_depth_sums(mesh_depth, depth.float(), args.min_depth, args.max_depth)]
            if gt_mesh_depth is not None:
                sums.append(_mesh_depth_sums(mesh_depth, gt_mesh_depth, args.min_depth, args.max_depth))
            mesh_sums.append(torch.cat(sums))
            per_source = []
            for s in color_sources:
                r = mesh_texture_renderer if s == "texture" and mesh_texture_renderer is not None else mesh_renderer
                mesh_picture, _, mesh_face = r.render_color(poses[i] if poses is not None else gt_c2w, source=s)
                if mesh_color_hook is not None:
                    mesh_color_hook(i, s, mesh_picture)
                per_source.append(_mesh_color_vector(mesh_picture, color, mesh_face, with_ms_ssim))
            if per_source:
                color_vectors.append(torch.stack(per_source))
        row = eval_frame(mapper, frame, color, depth, args.min_depth, args.max_depth, renderer=renderer,
                         with_ms_ssim=with_ms_ssim, exposure_aware=exposure_aware, exposure_gates=exposure_gates,
                         exposure_events=exposure_events)
        if exposure_aware:
            exposure_rows.append({"frame": i, "psnr": row["psnr"], **{k: row.pop(k) for k in EXPOSURE_ROW_KEYS}})
        row["frame"] = i
        row["iter"] = int(getattr(mapper, "iter", 0))
        rows.append(row)
    if gt_cull is not None and rows:
        cv, cf = gt_cull.mesh()
        if cf.shape[0] == 0:
            raise ValueError(f"rtg_slam_amd.evaluation: no face of the GT mesh was seen within a tolerance of "
                             f"{gt_cull.tolerance:g} m over {gt_cull.frames} frames; is the mesh in the frame the poses map into?")
        gt_points = sample_mesh_points(cv, cf, len(gt_points) if gt_points is not None else 1_000_000, 0, mapper.device)
    if gt_points is not None and rows:
        with torch.no_grad():
            rec = mapper.opt.gaussian_data("all")["xyz"] if rec_points is None else rec_points
            rows[-1].update(eval_pcd(rec, gt_points, dist_thres, transform, sample_nums, generator))
    res = {"rows": rows, "mean": metrics_mean_row(rows)}
    if exposure_aware:
        keys = [k for k in ("psnr",) + EXPOSURE_ROW_KEYS if k != "code" and exposure_rows and exposure_rows[0][k] is not None]
        res["exposure_rows"] = exposure_rows
        res["exposure_mean"] = {k: float(np.mean([r[k] for r in exposure_rows])) for k in keys}
        res["exposure_mean"]["frames_refused"] = sum(1 for r in exposure_rows if r["code"] != 0)
        res["exposure_seconds"] = sum(a.elapsed_time(b) for a, b in exposure_events) * 1e-3    # every frame's host read is behind
    if mesh_renderer is not None:
        n_pixels = int(cam.H) * int(cam.W)
        mesh_rows = []
        for i, v in enumerate(torch.stack(mesh_sums).cpu().tolist() if mesh_sums else []):       # the one host read
            row = {"frame": i, **_mesh_depth_result(v[:2], n_pixels)}
            if len(v) > 2:
                row.update(_mesh_depth_result(v[2:], n_pixels, "_gt"))
            mesh_rows.append(row)
        keys = [k for k in (mesh_rows[0] if mesh_rows else {}) if k != "frame"]
        res["mesh_depth_rows"] = mesh_rows
        res["mesh_depth_mean"] = {k: float(np.mean([r[k] for r in mesh_rows])) for k in keys}
    if color_sources:
        n_pixels = int(cam.H) * int(cam.W)
        color_rows = []
        for i, per_source in enumerate(torch.stack(color_vectors).cpu().tolist() if color_vectors else []):   # the one host read
            row = {"frame": i}
            for s, v in zip(color_sources, per_source):
                row.update(_mesh_color_result(v, n_pixels, with_ms_ssim, "_tex" if s == "texture" else ""))
            color_rows.append(row)
        keys = [k for k in (color_rows[0] if color_rows else {}) if k != "frame" and color_rows[0][k] is not None]
        res["mesh_color_rows"] = color_rows
        res["mesh_color_mean"] = {k: float(np.mean([r[k] for r in color_rows])) for k in keys}
    return res
