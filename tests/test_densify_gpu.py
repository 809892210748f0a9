"""The stable cloud's densification on the GPU: the rtgs_densify_discs kernel against the reference's own points
(tests/golden/densify_ref.npz) and against the restatement (tests/densify_reference.py), Mapping.save_densified after a short
synthetic run, and `slam --pcd-densify` then `metric` on a Replica-layout dataset with a GT mesh."""
import csv
import os

import numpy as np
import pytest
import torch

from rtg_slam_amd import io_formats as iof, slam_ops as so, synth
from tests import densify_reference as dr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-6


def _kernel(xyz, scales, rotations, cos, sin, sigma, levels):
    out = so.densify_discs(xyz.to(DEV), scales.to(DEV), rotations.to(DEV), cos, sin, sigma, levels)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("case", [0, 1, 2])
def test_kernel_matches_the_references_points(case):
    z = np.load(os.path.join(HERE, "golden", "densify_ref.npz"))
    sigma, C, L = (int(v) for v in z["cases"][case])
    t = lambda k: torch.from_numpy(z[k])
    out = _kernel(t("xyz"), t("scales"), t("rotations"), t(f"cos_{case}"), t(f"sin_{case}"), sigma, L)
    assert out.dtype == torch.float64 and out.shape == (z["xyz"].shape[0] * sigma * C * L, 6)
    assert dr.close(out[:, :3], z[f"points_{case}"]) <= TOL
    assert dr.close(out[:, 3:], z[f"normals_{case}"]) <= TOL


def _random_map(P, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(P, 3, generator=g) * 3.0
    s = torch.exp(torch.randn(P, 3, generator=g) * 0.8 - 3.0)
    kind = torch.randint(0, 4, (P,), generator=g)
    s[kind == 1, 1] = s[kind == 1, 0]                                      # a tie of two
    s[kind == 2, 2] = s[kind == 2, 0]
    s[kind == 3] = s[kind == 3, :1].repeat(1, 3)                          # all three equal
    q = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=1)
    return xyz, s, q


@pytest.mark.parametrize("sigma,C,L", [(1, 30, 5), (3, 7, 3), (1, 1, 1), (3, 13, 3)])
def test_kernel_matches_the_restatement_on_a_random_map(sigma, C, L):
    xyz, s, q = _random_map(50_000, seed=sigma * 100 + C)
    cos, sin = so.densify_theta(C, torch.Generator().manual_seed(C))
    out = _kernel(xyz, s, q, cos, sin, sigma, L)
    pts, nrm = dr.densify(xyz, s, q, cos, sin, sigma, L)
    assert out.shape == (50_000 * sigma * C * L, 6)
    assert torch.isfinite(out).all()
    assert dr.close(out[:, :3], pts) <= TOL
    assert dr.close(out[:, 3:], nrm) <= TOL
    print("bit-exact rows", int((out.float() == torch.cat([pts, nrm], 1)).all(1).sum()), "of", out.shape[0])


def test_kernel_edge_sizes_and_ranges():
    xyz, s, q = _random_map(1000, seed=3)
    cos, sin = so.densify_theta(30)
    for P in (0, 1):
        out = _kernel(xyz[:P], s[:P], q[:P], cos, sin, 1, 5)
        pts, nrm = dr.densify(xyz[:P], s[:P], q[:P], cos, sin, 1, 5)
        assert out.shape == (150 * P, 6) and dr.close(out, torch.cat([pts, nrm], 1)) <= TOL
    # a row range writes the rows of the whole call's range, into the head of `out`
    full = so.densify_discs(xyz.to(DEV), s.to(DEV), q.to(DEV), cos, sin, 1, 5)
    buf = torch.full((200 * 150, 6), 7.0, dtype=torch.float64, device=DEV)
    part = so.densify_discs(xyz.to(DEV), s.to(DEV), q.to(DEV), cos, sin, 1, 5, row_begin=333, row_end=500, out=buf)
    assert torch.equal(part, full[333 * 150:500 * 150])
    assert bool((buf[167 * 150:] == 7.0).all())                          # nothing written past the range
    with pytest.raises(RuntimeError):                                       # K = 3 * 30 * 30 > the kernel's limit
        so.densify_discs(xyz.to(DEV), s.to(DEV), q.to(DEV), *so.densify_theta(30), 3, 30)


def _half_replica():
    c = synth.REPLICA
    return synth.CameraSpec(c.H // 2, c.W // 2, c.fx / 2, c.fy / 2, (c.cx + 0.5) / 2 - 0.5, (c.cy + 0.5) / 2 - 0.5)


@pytest.fixture(scope="module")
def short_run():
    from rtg_slam_amd import mapping as mp, slam
    cam = _half_replica()
    frames = []
    for p in synth.trajectory(16, seed=21):
        d = synth.box_room_depth(cam, p)
        frames.append((d.to(DEV), synth.box_room_color(cam, p, d).to(DEV), p.numpy()))
    args = mp.replica_args(uniform_sample_num=10200, gaussian_update_iter=30, stable_confidence_thres=15.0,
                           unstable_time_window=24, max_depth=8.0, keyframe_trans_thes=0.25, seed=1)
    mapper = mp.Mapping(args, DEV, capacity=200_000)
    mapper, _, _ = slam.run_sequence(cam, iter(frames), args, DEV, mapper=mapper)
    assert mapper.get_stable_num > 0
    return mapper


def _row_err(got, want, K):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    e = (got - want).abs() / want.abs().amax(dim=-1, keepdim=True).clamp_min(1.0)
    return e.reshape(-1, K * 3).amax(dim=1)


@pytest.mark.parametrize("sigma,C,L", [(1, 30, 5), (3, 7, 3)])
def test_save_densified_matches_the_saved_stable_cloud(short_run, tmp_path, sigma, C, L):
    mapper = short_run
    base = str(tmp_path / "iter_0001")
    mapper.save_model(base, save_sibr=False, save_merge=False)
    gd = mapper.opt.gaussian_data("stable")
    own = {k: gd[k].detach().cpu().clone() for k in ("xyz", "scales", "rotations")}
    path = str(tmp_path / "pcd_densify.ply")
    n = mapper.save_densified(path, sigma, C, L, generator=torch.Generator().manual_seed(4))
    K = sigma * C * L
    P = mapper.get_stable_num
    assert n == K * P
    xyz, nrm = iof.load_point_cloud_ply(path)
    assert xyz.shape == (n, 3) and nrm.shape == (n, 3)
    cos, sin = so.densify_theta(C, torch.Generator().manual_seed(4))
    # the map's own activated rows (what the kernel was given): every point within the tolerance
    pts, nr = dr.densify(own["xyz"], own["scales"], own["rotations"], cos, sin, sigma, L)
    assert dr.close(xyz, pts) <= TOL and dr.close(nrm, nr) <= TOL
    # the _stable.ply saved at the same moment, activated by torch (exp, normalize) as the reference does
    m = iof.load_model_ply(base + "_stable.ply")
    assert np.array_equal(m["xyz"], own["xyz"].numpy())
    scales = torch.exp(torch.from_numpy(m["scaling"]).float())
    rots = torch.nn.functional.normalize(torch.from_numpy(m["rotation"]).float(), dim=1)
    pts_t, nr_t = dr.densify(torch.from_numpy(m["xyz"]).float(), scales, rots, cos, sin, sigma, L)
    err = torch.maximum(_row_err(xyz, pts_t, K), _row_err(nrm, nr_t, K))
    # a last-bit difference between the map's exp and torch's can order two near-equal scales the other way; such a row
    # swaps its ellipse axes (or its normal).  Every row whose axis order agrees is within the tolerance; the others are
    # near ties, relative gap of the reordered scales <= 1e-6
    same = (torch.sort(scales, dim=1, stable=True).indices == torch.sort(own["scales"], dim=1, stable=True).indices).all(1)
    print(f"rows {P}: axis order differs on {int((~same).sum())}, beyond tolerance {int((err > TOL).sum())}, "
          f"max error where the order agrees {float(err[same].max()):.3g}, scales bit-equal rows "
          f"{int((scales == own['scales']).all(1).sum())}")
    assert float(err[same].max()) <= TOL
    if (~same).any():
        srt = torch.sort(scales[~same], dim=1).values.double()
        gap = torch.minimum((srt[:, 1] - srt[:, 0]) / srt[:, 1], (srt[:, 2] - srt[:, 1]) / srt[:, 2])
        assert float(gap.max()) <= 1e-6
    # in chunks of 7 Gaussians (and a ragged last one): the same bytes as in one chunk
    path2 = str(tmp_path / "chunked.ply")
    assert mapper.save_densified(path2, sigma, C, L, generator=torch.Generator().manual_seed(4), chunk_points=7 * K + 1) == n
    assert open(path2, "rb").read() == open(path, "rb").read()


def test_save_densified_of_an_empty_stable_cloud_writes_no_file(tmp_path):
    from rtg_slam_amd import mapping as mp
    mapper = mp.Mapping(mp.replica_args(), DEV, capacity=1000)
    path = str(tmp_path / "pcd_densify.ply")
    assert mapper.save_densified(path) == 0 and not os.path.exists(path)


def _write_box_mesh(path):
    """The box room of tests/test_eval_gpu.py::_box_points as a binary PLY mesh (8 vertices, 12 triangles)."""
    v = np.array([[x, y, z] for x in (-2.5, 2.5) for y in (-1.5, 1.5) for z in (-3.0, 3.0)], dtype="<f4")
    q = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]])
    f = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])
    face = np.zeros(len(f), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    face["n"], face["i"] = 3, f
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 8\nproperty float x\nproperty float y\n"
                 b"property float z\nelement face 12\nproperty list uchar int vertex_indices\nend_header\n")
        fh.write(v.tobytes() + face.tobytes())


def test_slam_pcd_densify_then_metric(tmp_path):
    from tests import test_run_config_gpu as rc
    from rtg_slam_amd import __main__ as cli, config, datasets, evaluation
    scene = rc._write_dataset(str(tmp_path))
    _write_box_mesh(os.path.join(scene, "room0.ply"))
    save = os.path.join(str(tmp_path), "out")
    # the overrides of test_run_config_gpu.py with fewer samples per frame: 150 x the stable rows stays under 1 M points
    cfg = rc._config(str(tmp_path), scene, save)
    text = open(cfg).read()
    open(cfg, "w").write(text.replace("uniform_sample_num: 10200", "uniform_sample_num: 4000"))
    out = rc._run(["slam", "--config", cfg, "--pcd-densify"], 900)
    assert "pcd_densify skipped" not in out and "pcd_densify: " in out
    pcd = os.path.join(save, "save_model", "pcd_densify.ply")
    final = os.path.join(save, "save_model", f"frame_{rc.N:04d}")
    model = cli.filter_models(final, False, [])[0]
    n_stable = iof.load_model_ply(os.path.join(final, model))["xyz"].shape[0]
    xyz, nrm = iof.load_point_cloud_ply(pcd)
    assert n_stable > 0 and xyz.shape == (150 * n_stable, 3) and nrm.shape == xyz.shape
    assert xyz.shape[0] <= 1_000_000                                      # no random subsample in eval_pcd

    out = rc._run(["metric", "--config", cfg], 600)
    assert f"geometry eval ply: {pcd}" in out
    csvs = [n for n in os.listdir(save) if n.startswith(f"statis_frame_{rc.N}_iter_")]
    with open(os.path.join(save, csvs[0])) as f:
        rows = list(csv.DictReader(f))
    row = rows[-2]                                                         # the last frame's row carries the geometry
    args = config.load_config(cfg)
    v, fc = iof.load_mesh_ply(os.path.join(scene, "room0.ply"))
    gt, _ = iof.sample_mesh_surface(v, fc, 1_000_000)
    want = evaluation.eval_pcd(torch.from_numpy(xyz).to(DEV, torch.float32), gt, [0.03], datasets.read_pose_t0(args),
                               1_000_000)
    print(want)
    for k, w in want.items():
        assert abs(float(row[k]) - w) <= 1e-9 * max(1.0, abs(w)), (k, row[k], w)

    # without the flag: no file, the skip is logged
    save2 = os.path.join(str(tmp_path), "out2")
    out = rc._run(["slam", "--config", rc._config(str(tmp_path), scene, save2), "--frames", "3"], 600)
    assert "pcd_densify skipped" in out
    assert not os.path.exists(os.path.join(save2, "save_model", "pcd_densify.ply"))
