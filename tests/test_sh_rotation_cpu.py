"""rtg_slam_amd/sh_rotation.py (the matrices that turn SH bands 1..3 with a rotation) and the definition of rtgs_map_deform_sh
(tests/map_deform_sh_reference.py) without a device; and, in the CPU oracle, that a map deformed WITH its bands turned renders at
the moved pose what it rendered before - and does not with the bands left as they were.

The 1e-12 of the block properties is float64 round-off with three decades of margin: the least-squares solve over 40 directions
leaves orthogonality at 1e-15, the defining property at 2e-15 and the product rule at 8e-16."""
import functools

import numpy as np
import torch

from oracle import raster_oracle as ro
from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import sh_rotation as shr
from rtg_slam_amd import synth
from rtg_slam_amd.rgbd_align import se3_exp
from tests import map_deform_reference as mdr
from tests import map_deform_sh_reference as msr
from tests import raster_util as ru
from tests.test_map_deform_gpu import CAM, DELTA, POSE, ROOM, differing_pixels

F32 = np.float32
TOL = 1e-12


def rot(axis_angle):
    return se3_exp(np.concatenate([np.asarray(axis_angle, dtype=np.float64), np.zeros(3)]))[:3, :3]


ROTATIONS = {"axis": rot([0.0, 0.0, 0.7]),                                              # about an axis of the basis
             "small": rot(np.deg2rad(3.0) * np.array([0.6, 0.64, -0.48])),              # 3 degrees, the size of a correction
             "large": rot(np.deg2rad(120.0) * np.array([-0.48, 0.6, 0.64]))}            # about 120 degrees


def directions(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def colour(shs, dirs):
    """eval_sh_color in float64: shs [16,3] shown from every direction of dirs [P,3]."""
    P = dirs.shape[0]
    return ro.eval_sh_color(3, torch.from_numpy(np.broadcast_to(shs, (P, 16, 3)).copy()), torch.from_numpy(dirs)).numpy()


def turned(shs, blocks):
    out = np.array(shs, dtype=np.float64)
    for (first, n, _), M in zip(msr.BANDS, blocks):
        out[first:first + n] = M @ shs[first:first + n]
    return out


def test_blocks_are_orthogonal_turn_the_colour_and_multiply():
    dirs = directions(1000, seed=5)
    shs = np.random.default_rng(6).normal(size=(16, 3))
    for name, R in ROTATIONS.items():
        blocks = shr.sh_rotation_blocks(R)
        assert [m.shape for m in blocks] == [(3, 3), (5, 5), (7, 7)] and all(m.dtype == np.float64 for m in blocks)
        for M in blocks:
            assert np.abs(M @ M.T - np.eye(M.shape[0])).max() < TOL, name
        # the defining property, per band and through the rasterizer's own evaluation: from R d the turned coefficients show
        # what the original ones showed from d
        for Y, Yr, M in zip(shr.sh_basis(dirs), shr.sh_basis(dirs @ R.T), blocks):
            assert np.abs(Yr - Y @ M.T).max() < TOL, name
        assert np.abs(colour(turned(shs, blocks), dirs @ R.T) - colour(shs, dirs)).max() < TOL, name
    names = list(ROTATIONS)
    for a in names:
        for b in names:
            R1, R2 = ROTATIONS[a], ROTATIONS[b]
            for M12, M1, M2 in zip(shr.sh_rotation_blocks(R1 @ R2), shr.sh_rotation_blocks(R1), shr.sh_rotation_blocks(R2)):
                assert np.abs(M12 - M1 @ M2).max() < TOL, (a, b)


def test_sh_basis_is_the_rasterizers():
    """sh_basis restates the 15 higher basis functions of eval_sh_color: a unit coefficient picks one of them."""
    dirs = directions(50, seed=8)
    Y = np.concatenate(shr.sh_basis(dirs), axis=1)
    for k in range(15):
        shs = np.zeros((16, 3))
        shs[1 + k] = 1.0
        assert np.abs(colour(shs, dirs)[:, 0] - 0.5 - Y[:, k]).max() < 1e-15


def test_band_1_closed_form():
    """Band 1 is the basis (-y, z, -x) up to its constant: M1[i][j] = s_i s_j R[p_i][p_j]."""
    p, s = (1, 2, 0), (-1.0, 1.0, -1.0)
    for name, R in ROTATIONS.items():
        M1 = shr.sh_rotation_blocks(R)[0]
        want = np.array([[s[i] * s[j] * R[p[i], p[j]] for j in range(3)] for i in range(3)])
        assert np.abs(M1 - want).max() < TOL, name


def test_an_exact_identity_gives_exact_identities():
    for M, n in zip(shr.sh_rotation_blocks(np.eye(3)), (3, 5, 7)):
        assert np.array_equal(M, np.eye(n))
    R = np.eye(3)
    R[0, 1] = -0.0                                                               # compares equal to the identity's zero
    for M, n in zip(shr.sh_rotation_blocks(R), (3, 5, 7)):
        assert np.array_equal(M, np.eye(n))


def corrections():
    """Frames 0 and 3 the identity, 1 a pure translation, 2 and 4 general, 5 a rotation alone."""
    D = np.stack([np.eye(4)] * 6)
    D[1, :3, 3] = (0.1, -0.2, 0.05)
    D[2] = DELTA
    D[4] = se3_exp([0.3, -0.2, 0.5, 0.0, 0.1, 0.0])
    D[5, :3, :3] = ROTATIONS["large"]
    return D


def test_table_layout_flags_and_agreement_with_deform_table():
    D = corrections()
    table = shr.sh_rotation_table(D)
    assert table.dtype == np.float32 and table.shape == (6, 84) and table.flags["C_CONTIGUOUS"]
    assert table.strides[0] == 336 and 336 % 16 == 0
    assert table[:, 83].tolist() == [0.0, 0.0, 1.0, 0.0, 1.0, 1.0]              # a correction that only translates does not turn
    eye_row = np.concatenate([np.eye(n).reshape(-1) for n in (3, 5, 7)]).astype(F32)
    for f in range(6):
        blocks = shr.sh_rotation_blocks(D[f, :3, :3])
        want = np.concatenate([m.reshape(-1) for m in blocks]).astype(F32)     # float64, rounded once
        assert np.array_equal(table[f, :83], want), f
        if table[f, 83] == 0:
            assert np.array_equal(table[f, :83], eye_row)
    # the same frames turn as in the table of rtgs_map_deform: its quaternion is the identity's exactly where the flag is 0
    quat = lc.deform_table(D)[:, 12:16]
    assert np.array_equal((quat == np.array([1, 0, 0, 0], dtype=F32)).all(axis=1), table[:, 83] == 0)
    # frame by frame and all frames at once are the same numbers
    assert np.array_equal(shr.sh_rotation_table(D[4:5]), table[4:5])
    assert shr.sh_rotation_table(np.zeros((0, 4, 4))).shape == (0, 84)


def test_the_definition_against_a_float64_product():
    rng = np.random.default_rng(3)
    N = 500
    shs = (rng.normal(size=(N, 16, 3)) * 0.05).astype(F32)
    shs[::7, 5] = -0.0                                                           # M x would make these +0.0
    shs[3::7] = -0.0
    D = corrections()
    table = shr.sh_rotation_table(D)
    tick = rng.integers(-3, 6 + 5, size=N)
    tick[:8] = (-2, 0, 1, 2, 3, 4, 5, 9)
    f = np.clip(tick, 0, 5)
    got = msr.deform_sh(shs, tick.astype(np.int32), table)
    assert got.dtype == F32 and got.shape == shs.shape
    assert np.array_equal(msr.deform_sh(shs, tick.astype(np.int64), table).view(np.int32), got.view(np.int32))
    stays = table[f, 83] == 0
    assert stays.any() and (~stays).any()
    assert np.array_equal(got[stays].view(np.int32), shs[stays].view(np.int32))                # bit for bit, -0.0 included
    assert np.array_equal(got[:, 0].view(np.int32), shs[:, 0].view(np.int32))                  # the DC term of every row
    want = shs.astype(np.float64)
    for first, n, at in msr.BANDS:
        M = table[f, at:at + n * n].astype(np.float64).reshape(N, n, n)
        want[:, first:first + n] = np.einsum("rij,rjc->ric", M, shs[:, first:first + n].astype(np.float64))
    scale = np.abs(want[~stays, 1:]).max()
    assert np.abs(got[~stays].astype(np.float64) - want[~stays]).max() < 1e-6 * scale
    # ticks below 0 and beyond the table are clamped: row 0 uses frame 0 (stays), row 7 frame 5
    assert tick[0] < 0 and stays[0] and tick[7] > 5
    assert np.array_equal(got[7].view(np.int32), msr.deform_sh(shs[7:8], np.array([5]), table)[0].view(np.int32))
    assert not np.array_equal(got[7, 1:].view(np.int32), shs[7, 1:].view(np.int32))


# ---- render equivalence in the oracle ----

@functools.lru_cache(maxsize=None)
def sh_render_scene():
    """The scene of tests/test_map_deform_gpu.py::render_pair_scene with its higher SH bands KEPT -> (map, deformed map with the
    bands turned by the definition, deformed map with the bands as they were, settings at POSE, settings at DELTA POSE, tick,
    table, sh_table).  Callers do not change what they get."""
    g = synth.surface_gaussians(2000, CAM, seed=11, half=ROOM)
    g = {k: v.clone() for k, v in g.items()}
    raw8 = np.zeros((2000, 8), dtype=F32)
    raw8[:, 4:8] = g["rotations"].numpy()
    tick = np.random.default_rng(2).integers(0, 6, size=2000)
    D = np.broadcast_to(DELTA, (6, 4, 4))
    table, sh_table = lc.deform_table(D), shr.sh_rotation_table(D)
    x1, r1 = mdr.deform(g["xyz"].numpy(), raw8, tick, table)
    plain = dict(g)
    plain["xyz"] = torch.from_numpy(x1)
    q = torch.from_numpy(r1[:, 4:8])
    plain["rotations"] = q / q.norm(dim=1, keepdim=True)
    plain["normal"] = synth.normal_from_scale_rot(g["scales"], plain["rotations"])
    turned_map = dict(plain)
    turned_map["shs"] = torch.from_numpy(msr.deform_sh(g["shs"].numpy(), tick, sh_table))
    sets = [ro.make_settings(CAM.H, CAM.W, CAM.fx, CAM.fy, CAM.cx, CAM.cy,
                             viewmatrix=torch.from_numpy(np.linalg.inv(P)).float().t().contiguous()) for P in (POSE, DELTA @ POSE)]
    return g, turned_map, plain, sets[0], sets[1], tick, table, sh_table


@functools.lru_cache(maxsize=None)
def oracle_counts():
    """-> (pixels that differ with the bands turned, with the bands left, covered fraction), in the CPU oracle."""
    g, d, plain, s0, s1, *_ = sh_render_scene()
    out_a, _, _ = ru.oracle_run(s0, g)
    out_b, _, _ = ru.oracle_run(s1, d)
    out_c, _, _ = ru.oracle_run(s1, plain)
    with_turn, covered = differing_pixels(out_a, g["normal"], out_b, d["normal"])
    without, _ = differing_pixels(out_a, g["normal"], out_c, plain["normal"])
    return with_turn, without, covered


def test_render_equivalence_in_the_oracle():
    """The map at POSE against the deformed map at DELTA POSE (3 degrees, 5 cm), higher bands present.  Computed on the CPU: with
    the definition's rows 0 of 19 200 pixels differ by more than 1e-4; with the bands left as they were 19 168 do - the control
    that gives tests/test_map_deform_sh_gpu.py::test_render_equivalence its teeth."""
    g = sh_render_scene()[0]
    assert float(g["shs"][:, 1:].abs().max()) > 0                               # the scene has higher bands
    with_turn, without, covered = oracle_counts()
    pixels = CAM.H * CAM.W
    print(f"oracle: {with_turn} of {pixels} pixels differ by more than 1e-4 with the bands turned, {without} with the bands left; "
          f"{100 * covered:.1f} % of the picture is covered")
    assert covered > 0.5
    assert with_turn == 0
    assert without > 0.5 * covered * pixels
