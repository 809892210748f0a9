"""A triangle mesh of the map: TSDF fusion and marching tetrahedra on the HIP kernels of include/rtgs_slam.h, "meshing"
(csrc/tsdf.hip).  The reference has no mesher; this is the step the Gaussian-SLAM literature scores against the GT mesh:
depth rendered from the map (or the sensor's own), fused into a truncated signed distance volume, the zero level extracted.

    TsdfVolume        a dense axis-aligned grid (tsdf, weight, rgb planes, float32, x fastest) with integrate / extract_mesh
    SparseTsdfVolume  the same virtual grid with planes only for the 8 x 8 x 8 bricks near an observed surface
    mesh_from_map     walk a trajectory, fuse every `every`-th frame's rendered or sensor depth and colour, extract the mesh

The per-voxel rule and the extraction are restated in numpy in tests/tsdf_reference.py, the brick allocation in
tests/tsdf_sparse_reference.py; the kernels match both bit for bit.
There is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
import time
from types import SimpleNamespace
from typing import Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from . import _lib

MAX_BYTES = 16 << 30                 # default cap of a volume's planes (20 B per voxel)
BYTES_PER_VOXEL = 20
BRICK_BYTES = 10240                  # RTGS_TSDF_BRICK_BYTES: 5 planes of 8 x 8 x 8 float32


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _intrinsics(K) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) from a camera with those attributes, a 3x3 matrix or the four numbers."""
    if all(hasattr(K, n) for n in ("fx", "fy", "cx", "cy")):
        return float(K.fx), float(K.fy), float(K.cx), float(K.cy)
    a = np.asarray(K.detach().cpu().numpy() if torch.is_tensor(K) else K, dtype=np.float64)
    if a.shape == (3, 3):
        return float(a[0, 0]), float(a[1, 1]), float(a[0, 2]), float(a[1, 2])
    if a.shape == (4,):
        return tuple(float(x) for x in a)
    raise ValueError("rtg_slam_amd.meshing: K must be a 3x3 matrix, (fx, fy, cx, cy) or a camera with those attributes")


def _host_pose(c2w) -> np.ndarray:
    return np.asarray(c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else c2w, dtype=np.float64).reshape(4, 4)


def set_dense_form(on: bool) -> None:
    """Debug knob (include/rtgs_debug.h, rtgs_tsdf_set_dense): integrate with one thread per voxel and no block test.  The
    planes are identical either way.  Process-wide."""
    _lib.load().rtgs_tsdf_set_dense(int(bool(on)))


def _prepare_frame(dev, depth, color, K, c2w):
    """The checks and conversions integrate() shares -> (depth, colour as contiguous float32, H, W, (fx, fy, cx, cy), the 12
    floats of the world-to-camera matrix)."""
    for t in (depth, color):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("rtg_slam_amd.meshing: tensors must live on a HIP device; this build has no CPU path.")
    if color.dim() != 3 or color.shape[0] != 3:
        raise ValueError("rtg_slam_amd.meshing: color must be [3,H,W]")
    H, W = int(color.shape[1]), int(color.shape[2])
    if depth.numel() != H * W:
        raise ValueError(f"rtg_slam_amd.meshing: depth has {depth.numel()} values, expected {H * W} for a {H}x{W} frame")
    if depth.device != dev or color.device != dev:
        raise ValueError("rtg_slam_amd.meshing: the frame and the volume live on different devices")
    w2c = np.linalg.inv(_host_pose(c2w)).astype(np.float32)
    m = (C.c_float * 12)(*w2c[:3, :3].reshape(-1).tolist(), *w2c[:3, 3].tolist())
    return depth.detach().float().contiguous(), color.detach().float().contiguous(), H, W, _intrinsics(K), m


def _weld(keys, pos, col, return_keys):
    """Triangle corners (keys [3 F], pos, col [3 F, 3]) -> (vertices, faces, colors[, keys]): welded by key, in key order."""
    uk, inv = torch.unique(keys, sorted=True, return_inverse=True)
    # any holder of a key serves: equal keys carry bit-identical positions and colours
    first = torch.empty(uk.shape[0], dtype=torch.int64, device=keys.device)
    first.scatter_(0, inv, torch.arange(inv.shape[0], dtype=torch.int64, device=keys.device))
    out = (pos[first], inv.reshape(-1, 3).to(torch.int32), col[first])
    return out + (uk,) if return_keys else out


class TsdfVolume:
    """Dense TSDF grid: corner `lo`, dims (nx, ny, nz) = ceil((hi - lo) / voxel), planes tsdf = 1, weight = 0, rgb = 0."""

    def __init__(self, lo, hi, voxel: float, trunc: Optional[float] = None, max_weight: float = 64, device=None,
                 max_bytes: int = MAX_BYTES):
        lo = [float(x) for x in lo]
        hi = [float(x) for x in hi]
        voxel = float(voxel)
        if not voxel > 0 or any(not h > l for l, h in zip(lo, hi)):
            raise ValueError(f"rtg_slam_amd.meshing: need voxel > 0 and hi > lo, got voxel {voxel}, lo {lo}, hi {hi}")
        dims = tuple(max(2, int(math.ceil((h - l) / voxel - 1e-9))) for l, h in zip(lo, hi))
        self._setup(lo, dims, voxel, trunc, max_weight, max_bytes)
        dev = self._device(device)
        nx, ny, nz = dims
        self.tsdf = torch.ones(nz, ny, nx, dtype=torch.float32, device=dev)
        self.weight = torch.zeros(nz, ny, nx, dtype=torch.float32, device=dev)
        self.rgb = torch.zeros(3, nz, ny, nx, dtype=torch.float32, device=dev)
        self._scratch = None

    def _setup(self, lo, dims, voxel, trunc, max_weight, max_bytes):
        n = dims[0] * dims[1] * dims[2]
        size = n * BYTES_PER_VOXEL
        if size > max_bytes or n > 2 ** 31 - 1:
            raise ValueError(f"rtg_slam_amd.meshing: a {dims[0]} x {dims[1]} x {dims[2]} grid at voxel {voxel:g} m needs "
                             f"{size / 2 ** 30:.2f} GiB of planes, over the cap of {max_bytes / 2 ** 30:.2f} GiB; use a larger "
                             "voxel or smaller bounds")
        self.lo = tuple(float(np.float32(x)) for x in lo)
        self.dims = tuple(int(d) for d in dims)
        self.voxel = float(np.float32(voxel))
        self.trunc = float(np.float32(4 * voxel if trunc is None else trunc))
        self.max_weight = float(max_weight)
        if not self.trunc > 0 or not self.max_weight >= 1:
            raise ValueError("rtg_slam_amd.meshing: need trunc > 0 and max_weight >= 1")
        self._lo_c = (C.c_float * 3)(*self.lo)
        self.frames = 0

    @staticmethod
    def _device(device):
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("rtg_slam_amd.meshing: the volume must live on a HIP device; this build has no CPU path.")
        return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev

    @classmethod
    def from_tensors(cls, tsdf: torch.Tensor, weight: torch.Tensor, rgb: torch.Tensor, lo, voxel: float,
                     trunc: Optional[float] = None, max_weight: float = 64, max_bytes: int = MAX_BYTES) -> "TsdfVolume":
        """A volume over existing planes (tsdf, weight [nz,ny,nx], rgb [3,nz,ny,nx], float32, contiguous, on the device); they
        are used in place."""
        for t in (tsdf, weight, rgb):
            if not t.is_cuda:
                raise RuntimeError("rtg_slam_amd.meshing: tensors must live on a HIP device; this build has no CPU path.")
        if tsdf.dim() != 3 or weight.shape != tsdf.shape or tuple(rgb.shape) != (3,) + tuple(tsdf.shape):
            raise ValueError("rtg_slam_amd.meshing: planes must be tsdf, weight [nz,ny,nx] and rgb [3,nz,ny,nx]")
        for t in (tsdf, weight, rgb):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("rtg_slam_amd.meshing: planes must be contiguous float32")
        nz, ny, nx = (int(s) for s in tsdf.shape)
        if min(nx, ny, nz) < 1:
            raise ValueError("rtg_slam_amd.meshing: empty grid")
        self = cls.__new__(cls)
        self._setup([float(x) for x in lo], (nx, ny, nz), float(voxel), trunc, max_weight, max_bytes)
        self.tsdf, self.weight, self.rgb = tsdf, weight, rgb
        self._scratch = None
        return self

    @property
    def device(self):
        return self.tsdf.device

    @property
    def hi(self):
        return tuple(l + d * self.voxel for l, d in zip(self.lo, self.dims))

    def integrate(self, depth: torch.Tensor, color: torch.Tensor, K, c2w) -> None:
        """Fuse one frame: depth (H*W values: [H,W], [H,W,1] or [1,H,W]; metres, <= 0 = hole), color [3,H,W], K (see
        _intrinsics), c2w 4x4.  The world-to-camera matrix is the float64 inverse of c2w cast to float32."""
        dev = self.device
        d, c, H, W, (fx, fy, cx, cy), m = _prepare_frame(dev, depth, color, K, c2w)
        lib = _lib.load()
        need = lib.rtgs_tsdf_scratch_bytes(H, W)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        nx, ny, nz = self.dims
        with torch.cuda.device(dev):
            rc = lib.rtgs_tsdf_integrate(_p(self.tsdf), _p(self.weight), _p(self.rgb), nx, ny, nz, self._lo_c, self.voxel,
                                         self.trunc, self.max_weight, _p(d), _p(c), H, W, fx, fy, cx, cy, m, _p(self._scratch),
                                         _stream(dev))
        _lib.check(rc, "rtgs_tsdf_integrate")
        self.frames += 1

    def extract_mesh(self, min_weight: float = 1, return_keys: bool = False):
        """Marching tetrahedra over the cells whose 8 corners have weight >= min_weight -> (vertices [V,3] float32, faces
        [F,3] int32, colors [V,3] float32) on the device.  Vertices are welded by their 64-bit edge key and come in key order,
        faces in (cell, tetrahedron, triangle) order, wound so the normal points towards positive tsdf; two runs are bit-equal.
        return_keys adds the keys [V] int64.  A corner whose tsdf is exactly 0 is outside; the crossings of its edges then
        coincide with the corner (distinct indices, a face without area)."""
        dev = self.device
        lib = _lib.load()
        nx, ny, nz = self.dims
        n = nx * ny * nz
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.rtgs_tsdf_count(_p(self.tsdf), _p(self.weight), nx, ny, nz, float(min_weight), _p(counts),
                                           _stream(dev)), "rtgs_tsdf_count")
        incl = torch.cumsum(counts, 0, dtype=torch.int64)
        n_tri = int(incl[-1])
        offsets = incl - counts
        del incl
        keys = torch.empty(3 * n_tri, dtype=torch.int64, device=dev)
        pos = torch.empty(3 * n_tri, 3, dtype=torch.float32, device=dev)
        col = torch.empty(3 * n_tri, 3, dtype=torch.float32, device=dev)
        if n_tri > 0:
            with torch.cuda.device(dev):
                _lib.check(lib.rtgs_tsdf_emit(_p(self.tsdf), _p(self.weight), _p(self.rgb), nx, ny, nz, self._lo_c, self.voxel,
                                              float(min_weight), _p(counts), _p(offsets), n_tri, _p(keys), _p(pos), _p(col),
                                              _stream(dev)), "rtgs_tsdf_emit")
        del counts, offsets
        return _weld(keys, pos, col, return_keys)


class SparseTsdfVolume:
    """TsdfVolume's virtual grid - lo, dims = ceil((hi - lo) / voxel), voxel, the same voxel centres - with planes only for the
    8 x 8 x 8 bricks near an observed surface: a table of one int32 per brick (its slot or -1) and a pool of 10 240 B per
    allocated brick, [slot][tsdf, weight, r, g, b][z][y][x].  A brick without a slot reads as fresh (tsdf 1, weight 0, rgb 0).

    A frame allocates the bricks of the 27 neighbours of every in-band voxel (one the dense rule updates and whose
    sdf / trunc < 1), in ascending brick linear index after the earlier slots, and then updates, by the dense rule's float
    chain, every voxel of an allocated brick that the dense rule updates.  What a brick's voxels saw before it was allocated
    is lost.  So (tests/tsdf_sparse_reference.py is the definition, matched bit for bit):
      * a voxel of an allocated brick equals TsdfVolume's unless the dense voxel was updated before the brick was allocated;
      * after one frame into a fresh volume every allocated voxel equals the dense one;
      * after one frame the mesh equals the dense mesh exactly - a cell with a triangle has a corner with tsdf < 0, which was in
        band, so the bricks of all 8 corners were allocated in that frame.
    max_bytes caps the table plus the pool's capacity; the pool grows geometrically.  The device memory is allocated at the
    first frame.  There is no CPU path."""

    BRICK = 8
    GROWTH = 1.5

    def __init__(self, lo, hi, voxel: float, trunc: Optional[float] = None, max_weight: float = 64, device=None,
                 max_bytes: int = MAX_BYTES):
        lo = [float(x) for x in lo]
        hi = [float(x) for x in hi]
        voxel = float(voxel)
        if not voxel > 0 or any(not h > l for l, h in zip(lo, hi)):
            raise ValueError(f"rtg_slam_amd.meshing: need voxel > 0 and hi > lo, got voxel {voxel}, lo {lo}, hi {hi}")
        dims = tuple(max(2, int(math.ceil((h - l) / voxel - 1e-9))) for l, h in zip(lo, hi))
        self.brick_dims = tuple((d + self.BRICK - 1) // self.BRICK for d in dims)
        n_table = self.brick_dims[0] * self.brick_dims[1] * self.brick_dims[2]
        self.max_bytes = int(max_bytes)
        if max(dims) > 2 ** 24 or n_table > 2 ** 31 - 1 or 4 * n_table > self.max_bytes:
            raise ValueError(f"rtg_slam_amd.meshing: a {dims[0]} x {dims[1]} x {dims[2]} grid at voxel {voxel:g} m needs a brick "
                             f"table of {4 * n_table / 2 ** 30:.2f} GiB, over the cap of {self.max_bytes / 2 ** 30:.2f} GiB (or "
                             "over 2^24 voxels on an axis); use a larger voxel or smaller bounds")
        self.lo = tuple(float(np.float32(x)) for x in lo)
        self.dims = dims
        self.voxel = float(np.float32(voxel))
        self.trunc = float(np.float32(4 * voxel if trunc is None else trunc))
        self.max_weight = float(max_weight)
        if not self.trunc > 0 or not self.max_weight >= 1:
            raise ValueError("rtg_slam_amd.meshing: need trunc > 0 and max_weight >= 1")
        self._lo_c = (C.c_float * 3)(*self.lo)
        self.device = TsdfVolume._device(device)
        self.frames = 0
        self.n_bricks = 0
        self._n_table = n_table
        self._table = self._flags = self._scratch = None
        self._pool = self._coords = None

    @property
    def hi(self):
        return tuple(l + d * self.voxel for l, d in zip(self.lo, self.dims))

    @property
    def capacity(self) -> int:
        """Bricks the pool holds without growing."""
        return 0 if self._pool is None else int(self._pool.shape[0])

    @property
    def pool_bytes(self) -> int:
        return self.capacity * BRICK_BYTES

    @property
    def bytes(self) -> int:
        """What max_bytes caps: the brick table and the pool's capacity."""
        return 4 * self._n_table + self.pool_bytes

    @property
    def dense_bytes(self) -> int:
        """What TsdfVolume's planes would take over the same grid."""
        return self.dims[0] * self.dims[1] * self.dims[2] * BYTES_PER_VOXEL

    @property
    def brick_coords(self) -> torch.Tensor:
        """[n_bricks, 3] int32: (bx, by, bz) in slot order."""
        if self._coords is None:
            return torch.zeros(0, 3, dtype=torch.int32, device=self.device)
        return self._coords[:self.n_bricks]

    def _ensure_table(self):
        if self._table is None:
            self._table = torch.full((self._n_table,), -1, dtype=torch.int32, device=self.device)
            self._flags = torch.empty(self._n_table, dtype=torch.int32, device=self.device)

    def _grow(self, need: int):
        """Make room for `need` bricks: at least GROWTH times the old capacity, as far as max_bytes allows; one copy."""
        if need <= self.capacity:
            return
        room = (self.max_bytes - 4 * self._n_table) // BRICK_BYTES
        if need > room:
            raise ValueError(f"rtg_slam_amd.meshing: the frame needs {need} bricks, {need * BRICK_BYTES / 2 ** 20:.2f} MiB of pool "
                             f"and {4 * self._n_table / 2 ** 20:.2f} MiB of brick table, over the cap of "
                             f"{self.max_bytes / 2 ** 20:.2f} MiB; raise max_bytes, or use a larger voxel or smaller bounds")
        cap = min(room, max(need, int(math.ceil(self.capacity * self.GROWTH))))
        pool = torch.empty(cap, 5, self.BRICK, self.BRICK, self.BRICK, dtype=torch.float32, device=self.device)
        coords = torch.empty(cap, 3, dtype=torch.int32, device=self.device)
        if self.n_bricks:
            pool[:self.n_bricks] = self._pool[:self.n_bricks]
            coords[:self.n_bricks] = self._coords[:self.n_bricks]
        self._pool, self._coords = pool, coords

    def integrate(self, depth: torch.Tensor, color: torch.Tensor, K, c2w) -> None:
        """TsdfVolume.integrate's arguments and checks.  Three launches - mark, allocate, integrate - with ONE host
        synchronisation between the first two: the host reads the number of new bricks to grow the pool (meshing is offline;
        mesh_from_map synchronises per frame anyway).  A frame that would take the table plus the pool over max_bytes raises
        ValueError before anything of it is written."""
        dev = self.device
        d, c, H, W, (fx, fy, cx, cy), m = _prepare_frame(dev, depth, color, K, c2w)
        lib = _lib.load()
        self._ensure_table()
        need = lib.rtgs_tsdf_scratch_bytes(H, W)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        nx, ny, nz = self.dims
        with torch.cuda.device(dev):
            _lib.check(lib.rtgs_tsdf_sparse_mark(_p(self._table), _p(self._flags), nx, ny, nz, self._lo_c, self.voxel, self.trunc,
                                                 _p(d), _p(c), H, W, fx, fy, cx, cy, m, _p(self._scratch), _stream(dev)),
                       "rtgs_tsdf_sparse_mark")
            incl = torch.cumsum(self._flags, 0, dtype=torch.int64)
            n_new = int(incl[-1])                                                # the frame's one synchronisation
            if n_new:
                self._grow(self.n_bricks + n_new)
                offsets = incl - self._flags
                _lib.check(lib.rtgs_tsdf_sparse_allocate(_p(self._table), _p(self._flags), _p(offsets), nx, ny, nz, self.n_bricks,
                                                         n_new, self.capacity, _p(self._coords), _p(self._pool), _stream(dev)),
                           "rtgs_tsdf_sparse_allocate")
                self.n_bricks += n_new
                del offsets
            del incl
            if self.n_bricks:
                _lib.check(lib.rtgs_tsdf_sparse_integrate(_p(self._pool), _p(self._coords), self.n_bricks, nx, ny, nz, self._lo_c,
                                                          self.voxel, self.trunc, self.max_weight, H, W, fx, fy, cx, cy, m,
                                                          _p(self._scratch), _stream(dev)), "rtgs_tsdf_sparse_integrate")
        self.frames += 1

    def extract_mesh(self, min_weight: float = 1, return_keys: bool = False):
        """TsdfVolume.extract_mesh's contract on the virtual grid: keys are (64-bit virtual linear index) * 7 + direction - 1,
        vertices welded and in key order, faces in (virtual cell linear index, tetrahedron, triangle) order.  The kernels walk
        the allocated bricks, so triangles leave in slot order and are sorted stably by their cell here.  A corner in a brick
        without a slot has weight 0, so min_weight must be > 0."""
        if not float(min_weight) > 0:
            raise ValueError("rtg_slam_amd.meshing: the sparse volume needs min_weight > 0 (unallocated bricks have weight 0)")
        dev = self.device
        empty = (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev),
                 torch.zeros(0, 3, dtype=torch.float32, device=dev))
        if self.n_bricks == 0:
            return empty + (torch.zeros(0, dtype=torch.int64, device=dev),) if return_keys else empty
        lib = _lib.load()
        nx, ny, nz = self.dims
        counts = torch.empty(self.n_bricks * self.BRICK ** 3, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.rtgs_tsdf_sparse_count(_p(self._pool), _p(self._coords), _p(self._table), self.n_bricks, nx, ny, nz,
                                                  float(min_weight), _p(counts), _stream(dev)), "rtgs_tsdf_sparse_count")
        incl = torch.cumsum(counts, 0, dtype=torch.int64)
        n_tri = int(incl[-1])
        offsets = incl - counts
        del incl
        cells = torch.empty(n_tri, dtype=torch.int64, device=dev)
        keys = torch.empty(3 * n_tri, dtype=torch.int64, device=dev)
        pos = torch.empty(3 * n_tri, 3, dtype=torch.float32, device=dev)
        col = torch.empty(3 * n_tri, 3, dtype=torch.float32, device=dev)
        if n_tri > 0:
            with torch.cuda.device(dev):
                _lib.check(lib.rtgs_tsdf_sparse_emit(_p(self._pool), _p(self._coords), _p(self._table), self.n_bricks, nx, ny, nz,
                                                     self._lo_c, self.voxel, float(min_weight), _p(counts), _p(offsets), n_tri,
                                                     _p(cells), _p(keys), _p(pos), _p(col), _stream(dev)), "rtgs_tsdf_sparse_emit")
        del counts, offsets
        # a cell's triangles are adjacent and in (tetrahedron, triangle) order already: a stable sort by cell finishes the order
        order = torch.sort(cells, stable=True).indices
        del cells
        corner = (order[:, None] * 3 + torch.arange(3, dtype=torch.int64, device=dev)[None, :]).reshape(-1)
        return _weld(keys[corner], pos[corner], col[corner], return_keys)

    def to_dense(self, window=None):
        """(tsdf, weight [wz,wy,wx], rgb [3,wz,wy,wx]) of the virtual grid, bricks without a slot fresh; window = ((x0, x1),
        (y0, y1), (z0, z1)) in voxels restricts it to a box.  Refuses a result over max_bytes.  For tests and debugging."""
        window = tuple((0, n) for n in self.dims) if window is None else tuple((int(a), int(b)) for a, b in window)
        if len(window) != 3 or any(not 0 <= a < b <= n for (a, b), n in zip(window, self.dims)):
            raise ValueError(f"rtg_slam_amd.meshing: window {window} is not a box of the {self.dims} grid")
        wx, wy, wz = (b - a for a, b in window)
        size = wx * wy * wz * BYTES_PER_VOXEL
        if size > self.max_bytes:
            raise ValueError(f"rtg_slam_amd.meshing: a dense copy of {wx} x {wy} x {wz} voxels needs {size / 2 ** 30:.2f} GiB, over "
                             f"the cap of {self.max_bytes / 2 ** 30:.2f} GiB; pass a smaller window")
        dev = self.device
        tsdf = torch.ones(wz, wy, wx, dtype=torch.float32, device=dev)
        weight = torch.zeros(wz, wy, wx, dtype=torch.float32, device=dev)
        rgb = torch.zeros(3, wz, wy, wx, dtype=torch.float32, device=dev)
        if self.n_bricks:
            w6 = (C.c_int32 * 6)(*[v for ab in window for v in ab])
            with torch.cuda.device(dev):
                _lib.check(_lib.load().rtgs_tsdf_sparse_to_dense(_p(self._pool), _p(self._table), *self.dims, w6, _p(tsdf),
                                                                 _p(weight), _p(rgb), _stream(dev)),
                           "rtgs_tsdf_sparse_to_dense")
        return tsdf, weight, rgb


def map_bounds(mapper, pad: float):
    """The bounding box of the map's Gaussian centres, padded by `pad` on every side -> (lo, hi)."""
    xyz = mapper.opt.gaussian_data("all")["xyz"].detach()
    if xyz.shape[0] == 0:
        raise ValueError("rtg_slam_amd.meshing: the map holds no Gaussians")
    lo, hi = xyz.min(0).values.cpu().tolist(), xyz.max(0).values.cpu().tolist()
    return [l - pad for l in lo], [h + pad for h in hi]


def cull_unseen(vertices, faces, colors, cam, poses, tolerance: float, transform=None, near: Optional[float] = None):
    """Remove the surface no pose could see -> (vertices, faces, colors, stats).  At every pose (c2w; `transform @ c2w` is the
    camera in the mesh's frame) the mesh is rendered (evaluation.MeshRenderer) and its own vertices are tested against that
    render (evaluation.VisibilityCull.add): a vertex is seen when it projects into a pixel whose rendered depth is not more
    than `tolerance` metres in front of it.  A face stays when some pose saw each of its three corners (mesh_ops.keep_faces;
    colours carried, colors may be None).  Visibility is decided per VERTEX, not by which faces won a pixel: at fine voxels
    most faces cover no pixel centre, and a face-map rule would punch holes into visible surface.  stats: "tolerance",
    "poses", "F_removed", "V_removed", "render_s" (device time of the renders) and "cull_s" (of the vertex tests)."""
    from . import evaluation, mesh_ops
    kw = {} if near is None else {"near": near}
    renderer = evaluation.MeshRenderer(vertices, faces, cam, transform=transform, **kw)
    cull = evaluation.VisibilityCull(renderer.vertices, renderer.faces, cam, transform=transform, tolerance=tolerance,
                                     device=renderer.device)
    for c2w in poses:
        c2w = _host_pose(c2w)
        depth, _ = renderer.render(c2w)
        cull.add(depth, c2w)
    if colors is not None:
        colors = torch.as_tensor(colors).to(device=renderer.device)
    v, f, c = mesh_ops.keep_faces(renderer.vertices, renderer.faces, colors, cull.keep())
    rep = cull.report()
    stats = {"tolerance": cull.tolerance, "poses": cull.frames, "F_removed": int(renderer.faces.shape[0]) - int(f.shape[0]),
             "V_removed": int(renderer.vertices.shape[0]) - int(v.shape[0]), "render_s": renderer.seconds, "cull_s": rep["seconds"]}
    return v, f, c, stats


_cull_unseen = cull_unseen                        # mesh_from_map has a flag of that name


def mesh_from_map(mapper, cam, poses=None, stream: Optional[Iterable] = None, *, voxel: float = 0.01, depth_source: str = "render",
                  every: int = 1, bounds=None, trunc: Optional[float] = None, max_weight: float = 64, min_weight: float = 1,
                  args=None, device=None, max_bytes: int = MAX_BYTES, volume: str = "dense", min_component_faces: int = 0,
                  simplify_cell: float = 0.0, normals: bool = False, cull_unseen: bool = False,
                  cull_unseen_tolerance: Optional[float] = None, decimate: float = 0.0,
                  decimate_max_error: Optional[float] = None):
    """Fuse a trajectory into a TsdfVolume (volume "dense") or a SparseTsdfVolume ("sparse") and extract its mesh ->
    (vertices, faces, colors, report).

    depth_source "render": the map (mapper.global_params) rendered at every pose by the evaluation renderer - a Renderer whose
    opaque threshold is args.renderer_opaque_threshold_eval, as evaluate_sequence constructs it - under no_grad, so the
    rasterizer runs with its no-backward flag; the rendered `depth` and `render` are fused.  "sensor": the stream's own depth
    and colour.  `stream` yields (depth, colour [3,H,W], GT c2w) as run_sequence's does; frame i is placed at poses[i], or at
    its GT pose without poses; "render" needs poses or a stream, "sensor" a stream.  Every `every`-th frame is fused.
    bounds = (lo, hi); default: the box of the map's Gaussian centres padded by trunc.  report: voxel, trunc, dims, bounds,
    frames fused, V, F and the seconds spent rendering, integrating and extracting; with volume "sparse", and only then, also
    "volume", "bricks", "brick_share" (allocated / all), "pool_bytes" and "dense_bytes" (what the dense planes would take).

    Clean-up (rtg_slam_amd.mesh_ops), off by default and applied in this order: min_component_faces > 0 drops the connected
    components with fewer faces; simplify_cell > 0 (metres, larger than the voxel) clusters the vertices on a grid of that
    cell anchored at the volume's lo; normals=True adds the final mesh's vertex normals as a FIFTH result, (vertices, faces,
    colors, report, normals).  With any of the three on, the report's V and F are the final counts and it gains "V_raw",
    "F_raw", the removal's "components", "components_removed", "faces_removed" and "vertices_removed" (when it ran),
    "simplify_cell", "normals" and "cleanup_s".

    decimate in (0, 1) is the share of the faces to keep: after the removal and the clustering, mesh_ops.decimate collapses
    half-edges by quadric error down to floor(decimate * F) faces, F counted at that stage; decimate_max_error (metres)
    bounds the error of every collapse and may stop it above the target.  It counts as clean-up (the keys above, "cleanup_s"
    includes it), and the report gains, only then, "decimate", "decimate_max_error", "F_before_decimate", "decimate_rounds",
    "decimate_collapses", "decimate_target_reached" and "decimate_s".

    cull_unseen=True removes, after the extraction and before the clean-up, the surface no fused view could see (cull_unseen
    below, at the fused poses, cull_unseen_tolerance metres, default the voxel): the report's V and F are the counts after it
    and it gains "cull_unseen" (the tolerance), "F_unseen_removed", "V_unseen_removed", "cull_render_s" and, as with the
    clean-up, "V_raw" and "F_raw": the extracted counts."""
    from .mapping import Frame
    from .render import Renderer
    if volume not in ("dense", "sparse"):
        raise ValueError(f"rtg_slam_amd.meshing: mesh_from_map's volume must be 'dense' or 'sparse', got {volume!r}")
    if depth_source not in ("render", "sensor"):
        raise ValueError(f"rtg_slam_amd.meshing: depth_source must be 'render' or 'sensor', got {depth_source!r}")
    if depth_source == "sensor" and stream is None:
        raise ValueError("rtg_slam_amd.meshing: depth_source='sensor' needs the frame stream")
    if stream is None and poses is None:
        raise ValueError("rtg_slam_amd.meshing: need poses or a stream")
    min_component_faces, simplify_cell, normals = int(min_component_faces), float(simplify_cell), bool(normals)
    if simplify_cell != 0 and not simplify_cell > float(voxel):
        raise ValueError(f"rtg_slam_amd.meshing: simplify_cell {simplify_cell:g} m must be larger than the voxel ({float(voxel):g} m); "
                         "a cell that holds one vertex simplifies nothing")
    decimate = float(decimate)
    if not 0 <= decimate < 1:
        raise ValueError(f"rtg_slam_amd.meshing: decimate is the share of faces to keep, 0 (off) <= decimate < 1, got {decimate:g}")
    if decimate_max_error is not None and not (decimate > 0 and float(decimate_max_error) > 0):
        raise ValueError("rtg_slam_amd.meshing: decimate_max_error must be > 0 and needs decimate > 0")
    every = max(1, int(every))
    trunc = 4 * float(voxel) if trunc is None else float(trunc)
    if device is None:
        device = mapper.device
    device = torch.device(device)
    lo, hi = map_bounds(mapper, trunc) if bounds is None else bounds
    vol = (SparseTsdfVolume if volume == "sparse" else TsdfVolume)(lo, hi, voxel, trunc, max_weight, device, max_bytes)
    renderer = None
    if depth_source == "render":
        args = mapper.args if args is None else args
        eval_args = SimpleNamespace(**vars(args))
        eval_args.renderer_opaque_threshold = float(getattr(args, "renderer_opaque_threshold_eval", 0.5))
        renderer = Renderer(eval_args)
    t_render = t_integrate = 0.0
    fused_poses = []
    source = stream if stream is not None else ((None, None, p) for p in poses)
    for i, (depth, color, gt_c2w) in enumerate(source):
        if poses is not None and i >= len(poses):
            break
        if i % every:
            continue
        c2w = _host_pose(poses[i] if poses is not None else gt_c2w)
        if renderer is not None:
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            frame = Frame(cam, c2w, device, uid=i)
            with torch.no_grad():
                out = renderer.render(frame, {k: v.detach() for k, v in mapper.global_params.items()})
            depth, color = out["depth"], out["render"]
            torch.cuda.synchronize(device)
            t_render += time.perf_counter() - t0
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        vol.integrate(depth, color, cam, c2w)
        torch.cuda.synchronize(device)
        t_integrate += time.perf_counter() - t0
        fused_poses.append(c2w)
    t0 = time.perf_counter()
    vertices, faces, colors = vol.extract_mesh(min_weight)
    torch.cuda.synchronize(device)
    t_extract = time.perf_counter() - t0
    report: Dict = {"voxel": vol.voxel, "trunc": vol.trunc, "dims": list(vol.dims), "bounds": [list(vol.lo), list(vol.hi)],
                    "depth_source": depth_source, "every": every, "frames_fused": vol.frames, "V": int(vertices.shape[0]),
                    "F": int(faces.shape[0]), "render_s": t_render, "integrate_s": t_integrate, "extract_s": t_extract}
    if volume == "sparse":
        n_table = vol.brick_dims[0] * vol.brick_dims[1] * vol.brick_dims[2]
        report.update({"volume": "sparse", "bricks": vol.n_bricks, "brick_share": vol.n_bricks / n_table,
                       "pool_bytes": vol.pool_bytes, "dense_bytes": vol.dense_bytes})
    v_raw, f_raw = report["V"], report["F"]
    if cull_unseen:
        tolerance = float(vol.voxel if cull_unseen_tolerance is None else cull_unseen_tolerance)
        vertices, faces, colors, stats = _cull_unseen(vertices, faces, colors, cam, fused_poses, tolerance)
        report.update({"V_raw": v_raw, "F_raw": f_raw, "V": int(vertices.shape[0]), "F": int(faces.shape[0]),
                       "cull_unseen": stats["tolerance"],
                       "F_unseen_removed": f_raw - int(faces.shape[0]), "V_unseen_removed": v_raw - int(vertices.shape[0]),
                       "cull_render_s": stats["render_s"]})
    if min_component_faces > 0 or simplify_cell > 0 or normals or decimate > 0:
        from . import mesh_ops
        t0 = time.perf_counter()
        extra: Dict = {}
        if decimate > 0:
            vertices, faces, colors, _, stats = mesh_ops.clean_mesh(
                vertices, faces, colors, min_component_faces=min_component_faces, simplify_cell=simplify_cell, origin=vol.lo)
            torch.cuda.synchronize(device)
            t1 = time.perf_counter()
            f_before = int(faces.shape[0])
            vertices, faces, colors, dstats = mesh_ops.decimate(vertices, faces, colors, int(decimate * f_before), decimate_max_error)
            torch.cuda.synchronize(device)
            extra = {"decimate": decimate, "decimate_max_error": None if decimate_max_error is None else float(decimate_max_error),
                     "F_before_decimate": f_before, "decimate_rounds": dstats["rounds"], "decimate_collapses": dstats["collapses"],
                     "decimate_target_reached": dstats["target_reached"], "decimate_s": time.perf_counter() - t1}
            nrm = mesh_ops.vertex_normals(vertices, faces) if normals else None
        else:
            vertices, faces, colors, nrm, stats = mesh_ops.clean_mesh(
                vertices, faces, colors, min_component_faces=min_component_faces, simplify_cell=simplify_cell, origin=vol.lo,
                normals=normals)
        torch.cuda.synchronize(device)
        report.update({"V_raw": v_raw, "F_raw": f_raw, "V": int(vertices.shape[0]), "F": int(faces.shape[0]), **stats,
                       "simplify_cell": simplify_cell, "normals": normals, "cleanup_s": time.perf_counter() - t0, **extra})
        if normals:
            return vertices, faces, colors, report, nrm
    return vertices, faces, colors, report
