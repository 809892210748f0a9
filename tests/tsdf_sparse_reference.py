"""Plain-numpy restatement of the sparse brick TSDF volume (include/rtgs_slam.h, "meshing", rtgs_tsdf_sparse_*;
rtg_slam_amd.meshing.SparseTsdfVolume).  It reuses the arithmetic of tests/tsdf_reference.py - tr.integrate is the per-voxel
chain, tr.make_tets / tr.make_table the marching-tetrahedra cases - and adds what is new: which 8 x 8 x 8 bricks a frame
allocates, in which order, and which voxels it may update.  Used only by tests; the kernels are held to it bit for bit.

The virtual grid is the dense volume's: lo, dims (nx, ny, nz), voxel, centres lo + ((float)i + 0.5f) voxel, 64-bit linear index
(iz ny + iy) nx + ix.  Brick (bx, by, bz) covers voxels [8 bx, 8 bx + 8) x ... cut at the grid; brick dims are ceil(n / 8), the
brick linear index is (bz nby + by) nbx + bx.  An unallocated brick reads as a fresh volume (tsdf 1, weight 0, rgb 0).

One frame:
  1. a voxel is IN BAND when the dense chain would update it (steps 1-9: it projects into the image, its pixel's depth is > 0,
     sdf = d - zc >= -trunc) and, in float32, sdf / trunc < 1;
  2. every in-band voxel marks the bricks of its 27 neighbours (ix + dx, iy + dy, iz + dz), d in {-1, 0, 1}^3, inside the grid;
  3. marked bricks without a slot get one, in ascending brick linear index after all earlier slots, and start fresh;
  4. every voxel the dense rule updates (free space, s = 1, included) that lies in an allocated brick is updated by the same
     chain; voxels of unallocated bricks are not, so what was observed before a brick's allocation is lost.

What follows:
  * a voxel of an allocated brick equals the dense volume's bit for bit unless the dense voxel was updated before the brick was
    allocated (SparseVolume.lost records those);
  * after one frame into a fresh volume every allocated voxel equals the dense one;
  * after one frame the mesh equals the dense mesh exactly: a cell with a triangle has a corner with tsdf < 0, that corner was
    in band, and rule 2 allocated the bricks of all 8 corners in the same frame.

A SparseVolume may hold only a WINDOW of the virtual grid (brick-aligned, or cut at the grid) with the true voxel indices, so
that a grid no array can hold is still checked where the frame falls; it asserts that no in-band voxel touches the window's
inner faces, so nothing the full grid would allocate is missed."""
import numpy as np

from tests import tsdf_reference as tr

F = np.float32
BRICK = 8


def brick_dims(dims):
    return tuple((int(n) + BRICK - 1) // BRICK for n in dims)


class _true_indices:
    """tr.integrate asks tr.axis_centres for the x, y and z centres, in that order; inside this context the answers are the
    centres of the window's true indices, lo + ((float)(i0 + j) + 0.5f) voxel, the same float chain."""

    def __init__(self, offset):
        self.offset = list(offset)

    def __enter__(self):
        self.saved = tr.axis_centres
        pending = list(self.offset)

        def centres(lo, n, voxel):
            i0 = pending.pop(0)
            return F(lo) + (np.arange(i0, i0 + n, dtype=np.int64).astype(F) + F(0.5)) * F(voxel)

        tr.axis_centres = centres
        return self

    def __exit__(self, *exc):
        tr.axis_centres = self.saved


class SparseVolume:
    def __init__(self, lo, dims, voxel, trunc, max_weight=64.0, window=None):
        self.lo = tuple(F(x) for x in lo)
        self.dims = tuple(int(d) for d in dims)
        self.voxel, self.trunc, self.max_weight = F(voxel), F(trunc), F(max_weight)
        self.brick_dims = brick_dims(self.dims)
        self.window = tuple((0, n) for n in self.dims) if window is None else tuple((int(a), int(b)) for a, b in window)
        for (a, b), n in zip(self.window, self.dims):
            assert 0 <= a < b <= n and a % BRICK == 0 and (b % BRICK == 0 or b == n), "the window must be brick-aligned"
        self.offset = tuple(a for a, _ in self.window)
        self.shape = tuple(b - a for a, b in self.window)                     # (wx, wy, wz)
        self.tsdf, self.weight, self.rgb = tr.new_volume(self.shape)
        wb = brick_dims(self.shape)
        self.table = np.full((wb[2], wb[1], wb[0]), -1, np.int64)             # slot of the window's bricks, [bz][by][bx]
        self.brick_coords = np.zeros((0, 3), np.int32)                        # (bx, by, bz) of the virtual grid, slot order
        self.lost = np.zeros(self.tsdf.shape, bool)                           # dense would have updated it while unallocated
        self.frames = 0

    @property
    def n_bricks(self):
        return len(self.brick_coords)

    def allocated_voxels(self, table=None):
        """[wz, wy, wx] bool: the voxel's brick has a slot."""
        a = (self.table if table is None else table) >= 0
        for axis in range(3):
            a = np.repeat(a, BRICK, axis=axis)
        wx, wy, wz = self.shape
        return a[:wz, :wy, :wx]

    def _run(self, planes, depth, color, K, c2w):
        lo = [float(x) for x in self.lo]
        if any(self.offset):
            with _true_indices(self.offset):
                return tr.integrate(*planes, lo, self.voxel, self.trunc, self.max_weight, depth, color, K, c2w)
        return tr.integrate(*planes, lo, self.voxel, self.trunc, self.max_weight, depth, color, K, c2w)

    def integrate(self, depth, color, K, c2w):
        """One frame.  -> {"in_band", "new_bricks", "updated"}."""
        wx, wy, wz = self.shape
        # a fresh probe volume: the dense rule leaves weight 1 exactly where it updates and tsdf = (1 * 0 + s) / 1 = s there
        probe = tr.new_volume(self.shape)
        self._run(probe, depth, color, K, c2w)
        updates = probe[1] == 1
        in_band = updates & (probe[0] < 1)
        # rule 2: the 27 neighbours inside the grid, then the bricks they lie in
        near = in_band.copy()
        for axis in range(3):
            grown = near.copy()
            lo_part = [slice(None)] * 3
            hi_part = [slice(None)] * 3
            lo_part[axis], hi_part[axis] = slice(0, -1), slice(1, None)
            grown[tuple(hi_part)] |= near[tuple(lo_part)]
            grown[tuple(lo_part)] |= near[tuple(hi_part)]
            near = grown
        for axis, ((a, b), n) in enumerate(zip(self.window[::-1], self.dims[::-1])):          # arrays are [z][y][x]
            first, last = [slice(None)] * 3, [slice(None)] * 3
            first[axis], last[axis] = 0, -1
            assert a == 0 or not in_band[tuple(first)].any(), "an in-band voxel on an inner face of the window"
            assert b == n or not in_band[tuple(last)].any(), "an in-band voxel on an inner face of the window"
        wb = self.table.shape
        padded = np.zeros((wb[0] * BRICK, wb[1] * BRICK, wb[2] * BRICK), bool)
        padded[:wz, :wy, :wx] = near
        marked = padded.reshape(wb[0], BRICK, wb[1], BRICK, wb[2], BRICK).any(axis=(1, 3, 5))
        # rule 3: ascending brick linear index (the window's [bz][by][bx] order is the virtual grid's)
        new = marked & (self.table < 0)
        bz, by, bx = np.nonzero(new)
        self.table[bz, by, bx] = self.n_bricks + np.arange(len(bz))
        ob = [o // BRICK for o in self.offset]
        coords = np.stack([bx + ob[0], by + ob[1], bz + ob[2]], -1).astype(np.int32).reshape(-1, 3)
        self.brick_coords = np.concatenate([self.brick_coords, coords])
        # rule 4: the dense chain on a copy, kept where the brick has a slot
        allocated = self.allocated_voxels()
        work = (self.tsdf.copy(), self.weight.copy(), self.rgb.copy())
        self._run(work, depth, color, K, c2w)
        self.tsdf = np.where(allocated, work[0], self.tsdf)
        self.weight = np.where(allocated, work[1], self.weight)
        self.rgb = np.where(allocated[None], work[2], self.rgb)
        self.lost |= updates & ~allocated
        self.frames += 1
        return {"in_band": int(in_band.sum()), "new_bricks": int(len(bz)), "updated": int((updates & allocated).sum())}

    def to_dense(self):
        """(tsdf, weight, rgb) of the window; unallocated bricks are fresh."""
        return self.tsdf, self.weight, self.rgb

    def linear_index(self, iz, iy, ix):
        """64-bit virtual linear index of window-local indices."""
        nx, ny, _ = self.dims
        ox, oy, oz = self.offset
        return ((iz.astype(np.int64) + oz) * ny + (iy.astype(np.int64) + oy)) * nx + (ix.astype(np.int64) + ox)

    def extract(self, min_weight=1.0):
        """TsdfVolume.extract_mesh's contract on the virtual grid -> (vertices, faces, colors, keys): keys = virtual linear
        index * 7 + direction - 1 (int64), vertices welded and in key order, faces in (virtual cell linear index, tetrahedron,
        triangle) order.  The interpolation is tr.extract's with the true indices; on a whole grid the two agree bit for bit."""
        wx, wy, wz = self.shape
        nx, ny, _ = self.dims
        ox, oy, oz = self.offset
        tsdf, weight, rgb = self.tsdf, self.weight, self.rgb
        tets, table = tr.make_tets(), tr.make_table()
        sub = lambda a, c: a[(c >> 2) & 1:wz - 1 + ((c >> 2) & 1), (c >> 1) & 1:wy - 1 + ((c >> 1) & 1), (c & 1):wx - 1 + (c & 1)]
        ok = np.ones((wz - 1, wy - 1, wx - 1), bool)
        mask = np.zeros((wz - 1, wy - 1, wx - 1), np.int32)
        for c in range(8):
            ok &= sub(weight, c) >= F(min_weight)
            mask |= (sub(tsdf, c) < 0).astype(np.int32) << c
        act = ok & (mask > 0) & (mask < 255)
        iz, iy, ix = np.nonzero(act)
        mask = mask[act]
        cell = self.linear_index(iz, iy, ix)
        true = (ix + ox, iy + oy, iz + oz)
        order, keys, pos, col = [], [], [], []
        for t, tet in enumerate(tets):
            case = np.zeros(mask.shape, np.int32)
            for k in range(4):
                case |= ((mask >> tet[k]) & 1) << k
            for m in range(1, 15):
                sel = np.nonzero(case == m)[0]
                if sel.size == 0:
                    continue
                for j, tri in enumerate(table[t][m]):
                    kk, pp, cc = [], [], []
                    for a, b in tri:
                        bit = lambda c, axis: (c >> axis) & 1
                        la = (iz[sel] + bit(a, 2), iy[sel] + bit(a, 1), ix[sel] + bit(a, 0))
                        lb = (iz[sel] + bit(b, 2), iy[sel] + bit(b, 1), ix[sel] + bit(b, 0))
                        ta, tb = tsdf[la], tsdf[lb]
                        w = ta / (ta - tb)
                        p = []
                        for axis, i0 in enumerate(true):
                            pa = self.lo[axis] + ((i0[sel] + bit(a, axis)).astype(F) + F(0.5)) * self.voxel
                            pb = self.lo[axis] + ((i0[sel] + bit(b, axis)).astype(F) + F(0.5)) * self.voxel
                            p.append(pa + (pb - pa) * w)
                        kk.append(self.linear_index(*la) * 7 + ((a ^ b) - 1))
                        pp.append(np.stack(p, -1))
                        cc.append(np.stack([rgb[ch][la] + (rgb[ch][lb] - rgb[ch][la]) * w for ch in range(3)], -1))
                    order.append(np.stack([cell[sel], np.full(sel.size, t), np.full(sel.size, j)], -1))
                    keys.append(np.stack(kk, -1))
                    pos.append(np.stack(pp, 1))
                    col.append(np.stack(cc, 1))
        if not keys:
            return np.zeros((0, 3), F), np.zeros((0, 3), np.int32), np.zeros((0, 3), F), np.zeros(0, np.int64)
        order, keys, pos, col = np.concatenate(order), np.concatenate(keys), np.concatenate(pos), np.concatenate(col)
        perm = np.lexsort((order[:, 2], order[:, 1], order[:, 0]))
        keys, pos, col = keys[perm].reshape(-1), pos[perm].reshape(-1, 3), col[perm].reshape(-1, 3)
        assert pos.dtype == F and col.dtype == F and keys.dtype == np.int64
        uk, first, inv = np.unique(keys, return_index=True, return_inverse=True)
        return pos[first], inv.reshape(-1, 3).astype(np.int32), col[first], uk


def fuse_sparse(cam, frames, lo, dims, voxel, trunc, max_weight=64.0, window=None):
    """tr.fuse_reference for the sparse volume -> (SparseVolume, per-frame figures)."""
    vol = SparseVolume(lo, dims, voxel, trunc, max_weight, window)
    stats = [vol.integrate(np.asarray(depth, dtype=F).reshape(cam.H, cam.W), np.asarray(color, dtype=F),
                           (cam.fx, cam.fy, cam.cx, cam.cy), c2w) for depth, color, c2w in frames]
    return vol, stats


# the three frames of tests/test_mesh_gpu.py, shared by the sparse CPU and GPU tests (that file is marked gpu as a whole)
def three_frames():
    import math
    import torch
    from rtg_slam_amd import synth
    cam = synth.CameraSpec(120, 160, 100.0, 100.0, 79.5, 59.5)
    c, s = math.cos(math.radians(50.0)), math.sin(math.radians(50.0))
    yaw = torch.eye(4, dtype=torch.float64)
    yaw[:3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float64)
    traj = synth.trajectory(41, seed=3)
    out = []
    for i, p in enumerate((traj[0], traj[20], traj[40] @ yaw)):
        d = synth.box_room_depth(cam, p)
        col = synth.box_room_color(cam, p, d)
        if i == 1:
            d = synth.tum_noise(d, seed=4)
        out.append((d.reshape(cam.H, cam.W).contiguous(), col, p.numpy()))
    return cam, out


THREE_LO, THREE_VOXEL = (-2.4, -1.6, -2.4), 0.05
