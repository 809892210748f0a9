"""How the higher spherical-harmonic bands of a Gaussian turn with a rigid move of the map (numpy float64, host).

The rasterizer evaluates colour = sum_k c_k Y_k(d) + 0.5 with the 16 real basis functions of csrc/raster_chain.h (constants
RTGS_SH_C1, RTGS_SH_C2_*, RTGS_SH_C3_* of csrc/raster_common.h with their signs, coefficient order of shs[N,16,3];
oracle/raster_oracle.py::eval_sh_color restates it).  Band l (l = 1, 2, 3: coefficients 1..3, 4..8, 9..15) spans a space that a
rotation maps onto itself, so there is one matrix M_l with

    Y_l(R d) = M_l Y_l(d)    for every unit d,

orthogonal because the basis is orthonormal up to one factor per band.  A Gaussian whose coefficients become c' = M_l c, channel
by channel, shows from direction R d what it showed from d: c'^T Y(R d) = c^T M^T M Y(d).  The DC term does not turn.

    sh_rotation_blocks  (M1, M2, M3) of one rotation
    sh_rotation_table   the float32 table of rtgs_map_deform_sh (include/rtgs_slam.h), one row of 84 values per frame

The matrices are solved for, not derived: Y_l is evaluated at K fixed directions d_k and at R d_k, and M_l is the least-squares
solution of Y_l(R d_k) = M_l Y_l(d_k).  The directions are a Fibonacci lattice of 40 points, which keeps the 7 functions of band 3
well apart (condition number of the 40 x 7 system below 1.2), so the solve loses nothing: orthogonality, the defining property on
fresh directions and M(R1 R2) = M(R1) M(R2) all hold to a few 1e-16.  That is still not zero, hence the rule that
loop_closure.deform_table applies to its quaternion: a rotation that IS the identity gets the identity blocks exactly."""
from __future__ import annotations

from typing import Tuple

import numpy as np

# the constants of csrc/raster_common.h before their rounding to float32
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)
BAND_SIZES = (3, 5, 7)
TABLE_COLUMNS = 84                      # 9 + 25 + 49 matrix values, row-major, then the flag: 336 B a row, 16-B aligned
FLAG_COLUMN = 83
N_DIRECTIONS = 40


def sh_basis(dirs) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """dirs [..., 3] unit, float64 -> (Y1 [..., 3], Y2 [..., 5], Y3 [..., 7]): the basis functions 1..15 of the rasterizer."""
    d = np.asarray(dirs, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    y1 = np.stack([-SH_C1 * y, SH_C1 * z, -SH_C1 * x], axis=-1)
    y2 = np.stack([SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)], axis=-1)
    y3 = np.stack([SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4.0 * zz - xx - yy),
                   SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), SH_C3[4] * x * (4.0 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
                   SH_C3[6] * x * (xx - 3.0 * yy)], axis=-1)
    return y1, y2, y3


def _fibonacci_directions(n: int) -> np.ndarray:
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=-1)


_DIRS = _fibonacci_directions(N_DIRECTIONS)
_PINV = tuple(np.linalg.pinv(b) for b in sh_basis(_DIRS))          # [n, K] each: pinv(B) B = I_n


def _blocks_of(R: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """R [F, 3, 3] -> (M1 [F, 3, 3], M2 [F, 5, 5], M3 [F, 7, 7]), every frame solved in one product per band."""
    turned = np.matmul(_DIRS, np.transpose(R, (0, 2, 1)))          # [F, K, 3]: R d_k
    # rows of B are Y(d_k)^T, rows of B' are Y(R d_k)^T = Y(d_k)^T M^T:  M^T = pinv(B) B'
    return tuple(np.ascontiguousarray(np.transpose(np.matmul(p, b), (0, 2, 1))) for p, b in zip(_PINV, sh_basis(turned)))


def sh_rotation_blocks(R) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(M1 [3,3], M2 [5,5], M3 [7,7]) float64 with Y_l(R d) = M_l Y_l(d) for every unit d; R a 3 x 3 rotation.  An R that is
    exactly the identity returns exactly the identity blocks."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    if np.array_equal(R, np.eye(3)):
        return tuple(np.eye(n) for n in BAND_SIZES)
    return tuple(m[0] for m in _blocks_of(R[None]))


def sh_rotation_table(corrections) -> np.ndarray:
    """[n, 4, 4] float64 -> the table of rtgs_map_deform_sh, float32 [n, 84]: per frame M1, M2, M3 of the correction's rotation
    row-major (9 + 25 + 49 values), then a flag: 0.0 where the correction's 3 x 3 block is exactly the identity (the kernel does
    not write such a row; its blocks are the identity's), 1.0 otherwise.  Computed in float64 and rounded once."""
    D = np.asarray(corrections, dtype=np.float64).reshape(-1, 4, 4)
    n = D.shape[0]
    out = np.zeros((n, TABLE_COLUMNS), dtype=np.float64)
    at = 0
    for size in BAND_SIZES:
        out[:, at:at + size * size] = np.eye(size).reshape(-1)
        at += size * size
    turns = ~(D[:, :3, :3] == np.eye(3)).all(axis=(1, 2))
    if turns.any():
        blocks = _blocks_of(D[turns, :3, :3])
        out[turns, :FLAG_COLUMN] = np.concatenate([m.reshape(m.shape[0], -1) for m in blocks], axis=1)
        out[turns, FLAG_COLUMN] = 1.0
    return out.astype(np.float32)
