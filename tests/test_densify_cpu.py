"""The stable cloud's densification without a GPU: the restatement against the reference's own points
(tests/golden/densify_ref.npz), the point-cloud PLY writer and reader, metric's choice of geometry file and the
--pcd-densify option."""
import os

import numpy as np
import pytest
import torch

from rtg_slam_amd import __main__ as cli, io_formats as iof
from tests import densify_reference as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densify_ref.npz")
TOL = 1e-6


def _golden():
    return np.load(GOLDEN)


def test_golden_covers_the_tie_rows():
    z = _golden()
    s = z["scales"]
    srt = np.sort(s, axis=1)
    assert (srt[:, 1] == srt[:, 2]).sum() >= 12                  # equal in-plane scales
    assert ((srt[:, 0] == srt[:, 1]) & (srt[:, 1] == srt[:, 2])).sum() >= 12
    assert ((srt[:, 0] == srt[:, 1]) & (srt[:, 1] < srt[:, 2])).sum() >= 12
    assert [tuple(c) for c in z["cases"]] == [(1, 30, 5), (2, 7, 3), (3, 1, 1)]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_restatement_matches_the_references_densify(case):
    z = _golden()
    sigma, C, L = (int(v) for v in z["cases"][case])
    assert z[f"cos_{case}"].shape == (C,)
    pts, nrm = dr.densify(torch.from_numpy(z["xyz"]), torch.from_numpy(z["scales"]), torch.from_numpy(z["rotations"]),
                          torch.from_numpy(z[f"cos_{case}"]), torch.from_numpy(z[f"sin_{case}"]), sigma, L)
    want_p, want_n = z[f"points_{case}"], z[f"normals_{case}"]
    assert pts.shape == want_p.shape == (z["xyz"].shape[0] * sigma * L * C, 3)
    assert dr.close(pts, want_p) <= TOL
    assert dr.close(nrm, want_n) <= TOL


def test_restatement_frame_rule_on_ties():
    """Ties sort to the lower axis index: with R = I, the axes are the unit vectors in that order."""
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * 4)
    s = torch.tensor([[0.1, 1.0, 1.0], [1.0, 1.0, 0.1], [0.5, 0.5, 0.5], [0.2, 0.2, 0.9]])
    n, p0, p1, a0, a1 = dr.frames(s, q)
    e = torch.eye(3)
    assert torch.equal(torch.stack([n.argmax(1), p0.argmax(1), p1.argmax(1)], 1),
                       torch.tensor([[0, 1, 2], [2, 0, 1], [0, 1, 2], [0, 1, 2]]))
    assert torch.allclose(n[0], e[0]) and torch.equal(a0, torch.tensor([1.0, 1.0, 0.5, 0.2]))
    assert torch.equal(a1, torch.tensor([1.0, 1.0, 0.5, 0.9]))


def test_point_cloud_ply_round_trip_and_header(tmp_path):
    rng = np.random.default_rng(0)
    xyz, nrm = rng.standard_normal((1000, 3)), rng.standard_normal((1000, 3))
    path = str(tmp_path / "pcd.ply")
    assert iof.save_point_cloud_ply(path, xyz, nrm) == 1000
    raw = open(path, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\nelement vertex 1000\n"
              b"property double x\nproperty double y\nproperty double z\n"
              b"property double nx\nproperty double ny\nproperty double nz\nend_header\n")
    assert raw.startswith(header) and len(raw) == len(header) + 1000 * 48
    assert np.array_equal(np.frombuffer(raw[len(header):], "<f8").reshape(-1, 6), np.concatenate([xyz, nrm], 1))
    got_x, got_n = iof.load_point_cloud_ply(path)
    assert np.array_equal(got_x, xyz) and np.array_equal(got_n, nrm)
    # streamed in pieces: the same bytes
    path2 = str(tmp_path / "pcd2.ply")
    rows = np.concatenate([xyz, nrm], 1)
    with iof.PointCloudPlyWriter(path2, 1000) as w:
        for i in range(0, 1000, 333):
            w.write(rows[i:i + 333])
    assert open(path2, "rb").read() == raw
    with pytest.raises(ValueError):
        with iof.PointCloudPlyWriter(str(tmp_path / "short.ply"), 10) as w:
            w.write(rows[:5])


def test_empty_cloud_writes_no_file(tmp_path):
    path = str(tmp_path / "empty.ply")
    assert iof.save_point_cloud_ply(path, np.zeros((0, 3)), np.zeros((0, 3))) == 0
    assert not os.path.exists(path)


def test_reader_takes_float_or_double_in_any_order(tmp_path):
    rng = np.random.default_rng(1)
    n = 57
    cols = {c: rng.standard_normal(n) for c in ("nz", "x", "red", "z", "nx", "y", "ny")}
    dt = np.dtype([(c, "<f4" if c in ("x", "nz", "red") else "<f8") for c in cols])
    table = np.zeros(n, dt)
    for c in cols:
        table[c] = cols[c]
    path = str(tmp_path / "mixed.ply")
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\ncomment made here\nelement vertex %d\n" % n)
        for c in cols:
            f.write(b"property %s %s\n" % (b"float" if dt[c] == np.float32 else b"double", c.encode()))
        f.write(b"element face 0\nproperty list uchar int vertex_indices\nend_header\n")
        f.write(table.tobytes())
    xyz, nrm = iof.load_point_cloud_ply(path)
    assert np.array_equal(xyz, np.stack([table[c].astype(np.float64) for c in ("x", "y", "z")], 1))
    assert np.array_equal(nrm, np.stack([table[c].astype(np.float64) for c in ("nx", "ny", "nz")], 1))
    # a model file (float32, raw columns): its centres, and its (zero) normals
    model = str(tmp_path / "iter_0001_stable.ply")
    m_xyz = rng.standard_normal((9, 3)).astype(np.float32)
    iof.save_model_ply(model, m_xyz, np.zeros((9, 1, 3)), np.zeros((9, 15, 3)), np.zeros((9, 1)), np.zeros((9, 3)),
                       np.ones((9, 4)), np.ones(9))
    xyz, nrm = iof.load_point_cloud_ply(model)
    assert np.array_equal(xyz, m_xyz.astype(np.float64)) and np.array_equal(nrm, np.zeros((9, 3)))
    # ascii, without normals
    path = str(tmp_path / "ascii.ply")
    open(path, "w").write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float y\nproperty float x\nproperty float z\n"
                          "end_header\n1 2 3\n4 5 6\n")
    xyz, nrm = iof.load_point_cloud_ply(path)
    assert np.array_equal(xyz, [[2, 1, 3], [5, 4, 6]]) and nrm is None


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("present", [False, True])
def test_metric_geometry_source(tmp_path, flag, present):
    from types import SimpleNamespace
    base = str(tmp_path / "save_model")
    os.makedirs(base)
    select = os.path.join(base, "frame_0020", "iter_0100_stable.ply")
    if present:
        open(os.path.join(base, "pcd_densify.ply"), "wb").close()
    got = cli.geometry_ply(SimpleNamespace(pcd_densify=flag), base, select)
    assert got == (os.path.join(base, "pcd_densify.ply") if flag and present else select)
    assert cli.geometry_ply(SimpleNamespace(), base, select) == select       # a config without the key


def test_pcd_densify_option_parses():
    p = cli.build_parser()
    assert p.parse_args(["slam", "--config", "c.yaml", "--pcd-densify"]).pcd_densify is True
    assert p.parse_args(["slam", "--config", "c.yaml"]).pcd_densify is False
    with pytest.raises(SystemExit):
        p.parse_args(["metric", "--config", "c.yaml", "--pcd-densify"])


def test_densify_theta_is_the_references_draw():
    from rtg_slam_amd import slam_ops as so
    g = torch.Generator().manual_seed(5)
    cos, sin = so.densify_theta(30, g)
    theta = torch.rand(1, 30, generator=torch.Generator().manual_seed(5)) * torch.pi * 2
    assert cos.dtype == torch.float32 and cos.shape == (30,)
    assert torch.equal(cos, torch.cos(theta)[0]) and torch.equal(sin, torch.sin(theta)[0])
