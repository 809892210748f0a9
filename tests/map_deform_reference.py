"""The definition of rtgs_map_deform (include/rtgs_slam.h, csrc/map_deform.hip) in numpy float32: `deform` is what the kernel must
write, bit for bit.  numpy has no fused multiply-add, so `fmaf` builds one: the product of two float32 is exact in float64, the
float64 sum with the third operand is made ROUNDED TO ODD (the error of the addition, recovered exactly by a two-sum, sets the last
bit), and a value rounded to odd at 53 bits rounds to the same float32 as the exact one (53 >= 2 * 24 + 2).  Valid while nothing
overflows or goes subnormal - metres and unit quaternions do not."""
import numpy as np

F32 = np.float32
IDENTITY_ROW = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0], dtype=F32)


def fmaf(a, b, c):
    """Correctly rounded float32 a * b + c, elementwise."""
    a, b, c = (np.asarray(t, dtype=F32).astype(np.float64) for t in (a, b, c))
    p = a * b                                          # exact: 24 + 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                    # two-sum: p + c = s + err exactly
    bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
    even = (bits & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(F32)


def quat_mul(a, b):
    """Hamilton product a (x) b of (w, x, y, z) rows in the kernel's order of operations; a [4] or [N,4], b [N,4]."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    w = fmaf(-az, bz, fmaf(-ay, by, fmaf(-ax, bx, aw * bw)))
    x = fmaf(-az, by, fmaf(ay, bz, fmaf(ax, bw, aw * bx)))
    y = fmaf(az, bx, fmaf(ay, bw, fmaf(-ax, bz, aw * by)))
    z = fmaf(az, bw, fmaf(-ay, bx, fmaf(ax, by, aw * bz)))
    return np.stack([w, x, y, z], axis=-1).astype(F32)


def deform(xyz, raw8, tick, table):
    """-> (xyz', raw8') float32: xyz [N,3], raw8 [N,8], tick [N] of any integer dtype, table [n_frames,16] float32."""
    xyz, raw8 = np.array(xyz, dtype=F32), np.array(raw8, dtype=F32)
    table = np.asarray(table, dtype=F32).reshape(-1, 16)
    f = np.clip(np.asarray(tick).reshape(-1).astype(np.int64), 0, table.shape[0] - 1)
    rows = table[f]
    move = ~(rows == IDENTITY_ROW).all(axis=1)         # == : a -0.0 in the table is a zero
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.stack([fmaf(rows[:, 4 * r], x, fmaf(rows[:, 4 * r + 1], y, fmaf(rows[:, 4 * r + 2], z, rows[:, 4 * r + 3])))
                    for r in range(3)], axis=1)
    q = quat_mul(rows[:, 12:16], raw8[:, 4:8])
    xyz[move] = out[move]
    raw8[move, 4:8] = q[move]
    return xyz, raw8
