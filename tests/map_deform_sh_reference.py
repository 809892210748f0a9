"""The definition of rtgs_map_deform_sh (include/rtgs_slam.h, csrc/map_deform_sh.hip) in numpy float32: `deform_sh` is what the
kernel must write, bit for bit.  The fused multiply-add is the one of tests/map_deform_reference.py (valid while nothing overflows
or goes subnormal in the float64 sum - SH coefficients and the entries of orthogonal matrices do not)."""
import numpy as np

from tests.map_deform_reference import fmaf

F32 = np.float32
COLUMNS, FLAG = 84, 83
BANDS = ((1, 3, 0), (4, 5, 9), (9, 7, 34))            # (first coefficient, size n, offset of the n x n block in a table row)


def deform_sh(shs, tick, sh_table):
    """-> shs' float32 [N,16,3]: shs [N,16,3], tick [N] of any integer dtype, sh_table [n_frames,84] float32.  Per row: f = tick
    clamped to the table; a flag that compares equal to 0 leaves the row as it is; otherwise, per band, output i and channel,
    acc = M[i][n-1] x[n-1], then acc = fmaf(M[i][j], x[j], acc) for j = n-2 .. 0.  Coefficient 0 is never written."""
    shs = np.array(shs, dtype=F32).reshape(-1, 16, 3)
    table = np.asarray(sh_table, dtype=F32).reshape(-1, COLUMNS)
    f = np.clip(np.asarray(tick).reshape(-1)[:shs.shape[0]].astype(np.int64), 0, table.shape[0] - 1)
    rows = table[f]
    move = ~(rows[:, FLAG] == 0)                       # == : a -0.0 flag is a zero
    out = shs.copy()
    for first, n, at in BANDS:
        M = rows[:, at:at + n * n].reshape(-1, n, n)
        x = shs[:, first:first + n, :]                 # [N, n, 3]
        for i in range(n):
            acc = M[:, i, n - 1, None] * x[:, n - 1, :]
            for j in range(n - 2, -1, -1):
                acc = fmaf(np.broadcast_to(M[:, i, j, None], acc.shape), x[:, j, :], acc)
            out[:, first + i, :] = acc
    out[~move] = shs[~move]
    return out
