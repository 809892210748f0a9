"""A triangle mesh of the map: TSDF fusion and marching tetrahedra on the HIP kernels of include/rtgs_slam.h, "meshing"
(csrc/tsdf.hip).  The reference has no mesher; this is the step the Gaussian-SLAM literature scores against the GT mesh:
depth rendered from the map (or the sensor's own), fused into a truncated signed distance volume, the zero level extracted.

    TsdfVolume        a dense axis-aligned grid (tsdf, weight, rgb planes, float32, x fastest) with integrate / extract_mesh
    SparseTsdfVolume  the same virtual grid with planes only for the 8 x 8 x 8 bricks near an observed surface
    mesh_from_map     walk a trajectory, fuse every `every`-th frame's rendered or sensor depth and colour, extract the mesh
    texture_mesh      a per-face texture atlas of a mesh baked from colour views (TextureBaker; csrc/mesh_texture.hip)

The per-voxel rule and the extraction are restated in numpy in tests/tsdf_reference.py, the brick allocation in
tests/tsdf_sparse_reference.py, the texture bake in tests/mesh_texture_reference.py; the kernels match all three bit for bit.
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
BRICK_BYTES = _lib.CONSTANTS["RTGS_TSDF_BRICK_BYTES"]     # 5 planes of 8 x 8 x 8 float32

_p, _stream = _lib.ptr, _lib.stream


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


# ---------------------------------------------------------------------------------------------------------------------
# texture: a per-face atlas baked from colour views
# ---------------------------------------------------------------------------------------------------------------------

TEXTURE_MAX_LEVEL = _lib.CONSTANTS["RTGS_MESH_TEXTURE_MAX_LEVEL"]     # blocks of 2 .. 64 texels a side
TEXTURE_MAX_SIDE = _lib.CONSTANTS["RTGS_MESH_TEXTURE_MAX_SIDE"]


def texture_atlas_size(T: int) -> Tuple[int, int]:
    """(Wt, Ht) of an atlas of T block texels: k the smallest integer with 4^k >= T, Wt = 2^k, Ht = 2^k when T > 2^(2k-1), else
    2^(k-1) (Morton codes below 2^(2k-1) have y < 2^(k-1)).  T = 0 gives (1, 1)."""
    T = int(T)
    if T <= 0:
        return 1, 1
    k = 0
    while 4 ** k < T:
        k += 1
    return 1 << k, (1 << k) if 2 * T > 4 ** k else (1 << k) >> 1


class TextureBaker:
    """The texture atlas of a mesh and its bake (include/rtgs_slam.h, "mesh texture"; bit for bit
    tests/mesh_texture_reference.py).  Every face owns a square block of 2^l texels a side, l in 1..max_level the smallest
    level at which (2^l - 1) texels span its longest edge; the blocks are packed by Morton code in descending size, so they are
    aligned, disjoint and gap-free; the upper half of a block mirrors the triangle across its hypotenuse.

        baker = TextureBaker(vertices, faces, cam, texel=0.01, tolerance=0.02)
        for colour, c2w in views: baker.add(colour, c2w)          # renders the mesh's depth at c2w, bakes the view
        image, flags = baker.finish(colors)

    levels, capped [F] int32, offset [F] int64, origin [F,2] int32, uv [F,3,2] float32, texel_face [Ht,Wt] int32 and acc
    [Ht,Wt,4] float32 (w r, w g, w b, w) are device tensors; size = (Wt, Ht).  An atlas wider than 16384 raises ValueError.
    With F = 0 there is nothing to bake: size is (1, 1) and finish gives one black texel.  There is no CPU path."""

    def __init__(self, vertices, faces, cam, *, texel: float, tolerance: float, max_level: int = TEXTURE_MAX_LEVEL,
                 min_cos: float = 0.2, transform=None, near: Optional[float] = None):
        from . import evaluation
        texel, tolerance, min_cos, max_level = float(texel), float(tolerance), float(min_cos), int(max_level)
        if not (math.isfinite(texel) and texel > 0):
            raise ValueError(f"rtg_slam_amd.meshing: the texel must be finite and > 0, got {texel:g}")
        if not (math.isfinite(tolerance) and tolerance > 0):
            raise ValueError(f"rtg_slam_amd.meshing: the texture tolerance must be finite and > 0, got {tolerance:g}")
        if not 1 <= max_level <= TEXTURE_MAX_LEVEL:
            raise ValueError(f"rtg_slam_amd.meshing: the texture's max_level must lie in 1..{TEXTURE_MAX_LEVEL}, got {max_level}")
        if not 0 <= min_cos <= 1:
            raise ValueError(f"rtg_slam_amd.meshing: min_cos must lie in 0..1, got {min_cos:g}")
        kw = {} if near is None else {"near": near}
        self.renderer = evaluation.MeshRenderer(vertices, faces, cam, transform=transform, **kw)
        self.device = dev = self.renderer.device
        self.vertices, self.faces, self.cam = self.renderer.vertices, self.renderer.faces, cam
        self.texel = float(np.float32(texel))
        self.tolerance = float(np.float32(tolerance))
        self.max_level = max_level
        self.min_cos2 = float(np.float32(min_cos) * np.float32(min_cos))
        self.views = 0
        self._events = []
        self._seconds = 0.0
        F = int(self.faces.shape[0])
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        with torch.cuda.device(dev):
            t0.record()
            self.levels, self.capped = self._levels(self.texel)
            order = torch.sort(self.levels, descending=True, stable=True).indices
            size = torch.ones(F, dtype=torch.int64, device=dev) << (2 * self.levels[order].to(torch.int64))
            sorted_offset = torch.cumsum(size, 0) - size
            self.T = int(size.sum()) if F else 0
            Wt, Ht = texture_atlas_size(self.T)
            if Wt > TEXTURE_MAX_SIDE:
                raise ValueError(f"rtg_slam_amd.meshing: at a texel of {self.texel:g} m the blocks hold T = {self.T} texels, more than "
                                 f"a {TEXTURE_MAX_SIDE} x {TEXTURE_MAX_SIDE} atlas; {self._smallest_texel()}")
            self.size = (Wt, Ht)
            self.offset = torch.empty(F, dtype=torch.int64, device=dev)
            self.offset[order] = sorted_offset
            self.origin = torch.empty(F, 2, dtype=torch.int32, device=dev)
            self.uv = torch.empty(F, 3, 2, dtype=torch.float32, device=dev)
            self._record = torch.empty(F, 12, dtype=torch.float32, device=dev)       # per face: A, B - A, C - A, x0, y0, level
            self.texel_face = torch.full((Ht, Wt), -1, dtype=torch.int32, device=dev)
            self.acc = torch.zeros(Ht, Wt, 4, dtype=torch.float32, device=dev)
            if F:
                lib = _lib.load()
                order32 = order.to(torch.int32).contiguous()
                _lib.check(lib.rtgs_mesh_texture_face_layout(_p(self.vertices), _p(self.faces), _p(self.offset), _p(self.levels), F, Wt,
                                                             Ht, _p(self.origin), _p(self.uv), _p(self._record), _stream(dev)),
                           "rtgs_mesh_texture_face_layout")
                _lib.check(lib.rtgs_mesh_texture_texel_face(_p(sorted_offset), _p(order32), F, self.T, Wt, Ht, _p(self.texel_face),
                                                            _stream(dev)), "rtgs_mesh_texture_texel_face")
            t1.record()
        t1.synchronize()
        self.layout_s = t0.elapsed_time(t1) * 1e-3

    def _levels(self, texel: float):
        F, dev = int(self.faces.shape[0]), self.device
        levels = torch.empty(F, dtype=torch.int32, device=dev)
        capped = torch.empty(F, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().rtgs_mesh_texture_levels(_p(self.vertices), _p(self.faces), F, texel, self.max_level, _p(levels),
                                                            _p(capped), _stream(dev)), "rtgs_mesh_texture_levels")
        return levels, capped

    def _smallest_texel(self) -> str:
        """The words of the refusal: the smallest texel whose blocks fit, by bisection on the levels kernel (T falls as the
        texel grows), rounded up to three digits."""
        def fits(t):
            levels = self._levels(t)[0].to(torch.int64)
            return texture_atlas_size(int((torch.ones_like(levels) << (2 * levels)).sum()))[0] <= TEXTURE_MAX_SIDE
        lo = hi = self.texel
        for _ in range(64):
            hi *= 2
            if fits(float(np.float32(hi))):
                break
            lo = hi
        else:
            return "no texel fits this many faces"
        for _ in range(16):
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if fits(float(np.float32(mid))) else (mid, hi)
        digits = 2 - int(math.floor(math.log10(hi)))
        return f"the smallest texel that fits is {math.ceil(hi * 10 ** digits) / 10 ** digits:g} m"

    def add(self, color: torch.Tensor, c2w) -> None:
        """One view: color [3,H,W] float on the device at the camera's size, c2w its pose (`transform @ c2w` is the camera in
        the mesh's frame).  The mesh's depth is rendered at that pose and the view is added to acc.  No synchronisation."""
        c2w = _host_pose(c2w)
        depth = self.renderer.render(c2w)[0] if int(self.faces.shape[0]) else None
        self.bake(color, depth, c2w)

    def bake(self, color: torch.Tensor, depth: Optional[torch.Tensor], c2w) -> None:
        """add() with the depth map given: depth [H,W] float32 on the device, the mesh as c2w sees it (renderer.render)."""
        if not torch.is_tensor(color) or not color.is_cuda or (depth is not None and not depth.is_cuda):
            raise RuntimeError("rtg_slam_amd.meshing: tensors must live on a HIP device; this build has no CPU path.")
        H, W = int(self.cam.H), int(self.cam.W)
        if tuple(color.shape) != (3, H, W):
            raise ValueError(f"rtg_slam_amd.meshing: a view's colour must be [3,{H},{W}], got {tuple(color.shape)}")
        if color.device != self.device:
            raise ValueError("rtg_slam_amd.meshing: the view and the mesh live on different devices")
        c2w = _host_pose(c2w)
        self.views += 1
        if int(self.faces.shape[0]) == 0:
            return
        if tuple(depth.shape) != (H, W) or depth.dtype != torch.float32 or not depth.is_contiguous() or depth.device != self.device:
            raise ValueError(f"rtg_slam_amd.meshing: a view's depth must be a contiguous [{H},{W}] float32 tensor on the mesh's device")
        pose = self.renderer.transform @ c2w
        w2c = np.linalg.inv(pose).astype(np.float32)
        m = (C.c_float * 12)(*np.ascontiguousarray(w2c.reshape(-1)[:12]).tolist())
        o = (C.c_float * 3)(*pose[:3, 3].astype(np.float32).tolist())
        fx, fy, cx, cy = (float(np.float32(k)) for k in (self.cam.fx, self.cam.fy, self.cam.cx, self.cam.cy))
        color = color.detach().to(torch.float32).contiguous()
        Wt, Ht = self.size
        with torch.cuda.device(self.device):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = _lib.load().rtgs_mesh_texture_bake_view(_p(self.texel_face), Wt, Ht, _p(self._record), _p(color), _p(depth), H, W, fx,
                                                         fy, cx, cy, m, o, self.tolerance, self.min_cos2, _p(self.acc),
                                                         _stream(self.device))
            b.record()
        _lib.check(rc, "rtgs_mesh_texture_bake_view")
        self._events.append((a, b))

    @property
    def bake_seconds(self) -> float:
        """The device time of the bake launches so far (events, read here: synchronises on the last one)."""
        for a, b in self._events:
            b.synchronize()
            self._seconds += a.elapsed_time(b) * 1e-3
        self._events = []
        return self._seconds

    def finish(self, colors=None):
        """-> (image [Ht,Wt,3] uint8, flags [Ht,Wt] uint8: 0 unassigned, 1 assigned but seen by no view, 2 seen).  A texel no
        view saw takes the blend of its face's vertex colours (colors [V,3] in 0..1), 0.5 grey without them."""
        Wt, Ht = self.size
        dev = self.device
        image = torch.zeros(Ht, Wt, 3, dtype=torch.uint8, device=dev)
        flags = torch.zeros(Ht, Wt, dtype=torch.uint8, device=dev)
        if int(self.faces.shape[0]) == 0:
            return image, flags
        if colors is not None:
            if torch.is_tensor(colors) and not colors.is_cuda:
                raise RuntimeError("rtg_slam_amd.meshing: tensors must live on a HIP device; this build has no CPU path.")
            colors = torch.as_tensor(colors).detach().to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
            if colors.shape[0] != self.vertices.shape[0]:
                raise ValueError(f"rtg_slam_amd.meshing: {colors.shape[0]} colours for {self.vertices.shape[0]} vertices")
        with torch.cuda.device(dev):
            rc = _lib.load().rtgs_mesh_texture_finish(_p(self.texel_face), Wt, Ht, _p(self.faces), _p(self.levels), _p(self.origin),
                                                      C.c_void_p(0) if colors is None else _p(colors), _p(self.acc), _p(image),
                                                      _p(flags), _stream(dev))
        _lib.check(rc, "rtgs_mesh_texture_finish")
        return image, flags


def texture_mesh(vertices, faces, colors, cam, views, *, texel: float, tolerance: float, max_level: int = TEXTURE_MAX_LEVEL,
                 min_cos: float = 0.2, transform=None, near: Optional[float] = None):
    """Bake a texture for a mesh -> (image [Ht,Wt,3] uint8, uv [F,3,2] float32, stats), device tensors (TextureBaker has the
    rules).  views: an iterable of (colour [3,H,W] float device tensor, c2w); they are baked in the order given, one launch
    each after a render of the mesh's own depth, so the result is reproducible.  A texel takes part in a view when it is in
    front of the camera, its bilinear footprint lies in the image, the mesh's depth at its pixel is valid and not more than
    `tolerance` metres in front of it, and the squared cosine between its face and the ray is at least min_cos^2; the weight
    is cos^2 / z^2.  uv holds three texture coordinates per face, x right and y DOWN, in 0..1 of the image.  stats: "size" (Wt,
    Ht), "texels_assigned", "fill" (assigned / atlas), "texels_seen", "seen_share" (seen / assigned), "views", "faces_capped"
    (faces longer than (2^max_level - 1) texels, stretched), "levels" (faces per level, index 0 = level 1), "layout_s",
    "render_s" and "bake_s" (device time).  F = 0 gives a 1 x 1 black image."""
    baker = TextureBaker(vertices, faces, cam, texel=texel, tolerance=tolerance, max_level=max_level, min_cos=min_cos,
                         transform=transform, near=near)
    for color, c2w in views:
        baker.add(color, c2w)
    image, flags = baker.finish(colors)
    Wt, Ht = baker.size
    assigned, seen = int((flags > 0).sum()), int((flags == 2).sum())
    hist = torch.bincount(baker.levels.to(torch.int64), minlength=baker.max_level + 1)[1:baker.max_level + 1].tolist()
    stats = {"size": [Wt, Ht], "texels_assigned": assigned, "fill": assigned / (Wt * Ht), "texels_seen": seen,
             "seen_share": seen / assigned if assigned else 0.0, "views": baker.views, "faces_capped": int(baker.capped.sum()),
             "levels": hist, "layout_s": baker.layout_s, "render_s": baker.renderer.seconds, "bake_s": baker.bake_seconds}
    return image, baker.uv, stats


def mesh_from_map(mapper, cam, poses=None, stream: Optional[Iterable] = None, *, voxel: float = 0.01, depth_source: str = "render",
                  every: int = 1, bounds=None, trunc: Optional[float] = None, max_weight: float = 64, min_weight: float = 1,
                  args=None, device=None, max_bytes: int = MAX_BYTES, volume: str = "dense", min_component_faces: int = 0,
                  simplify_cell: float = 0.0, normals: bool = False, cull_unseen: bool = False,
                  cull_unseen_tolerance: Optional[float] = None, decimate: float = 0.0,
                  decimate_max_error: Optional[float] = None, texture_texel: float = 0.0,
                  texture_tolerance: Optional[float] = None, texture_max_level: int = TEXTURE_MAX_LEVEL):
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
    clean-up, "V_raw" and "F_raw": the extracted counts.

    texture_texel > 0 (metres) textures the FINAL mesh - after the cull, the clean-up, the decimation and the normals - with
    texture_mesh: the views are the map rendered again at the fused poses by the same evaluation renderer under no_grad (the
    sensor's colour is not used; call texture_mesh with views of your own for that), texture_tolerance defaults to the voxel.
    The result then gains a LAST element, the dict {"image", "uv", "stats"} of texture_mesh, and the report "texture_texel",
    "texture_size", "texture_fill", "texture_seen_share", "texture_views", "texture_faces_capped" and "texture_s".  With
    texture_texel = 0 the result and the report are what they are without the option."""
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
    texture_texel = float(texture_texel)
    if not (math.isfinite(texture_texel) and texture_texel >= 0):
        raise ValueError(f"rtg_slam_amd.meshing: texture_texel must be finite and >= 0 (0: off), got {texture_texel:g}")
    if not 1 <= int(texture_max_level) <= TEXTURE_MAX_LEVEL:
        raise ValueError(f"rtg_slam_amd.meshing: texture_max_level must lie in 1..{TEXTURE_MAX_LEVEL}, got {texture_max_level}")
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
    nrm = None
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
    result = (vertices, faces, colors, report) + ((nrm,) if normals else ())
    if texture_texel > 0:
        t0 = time.perf_counter()
        if renderer is None:
            args = mapper.args if args is None else args
            eval_args = SimpleNamespace(**vars(args))
            eval_args.renderer_opaque_threshold = float(getattr(args, "renderer_opaque_threshold_eval", 0.5))
            renderer = Renderer(eval_args)
        params = {k: v.detach() for k, v in mapper.global_params.items()}

        def views():
            for i, c2w in enumerate(fused_poses):
                with torch.no_grad():
                    out = renderer.render(Frame(cam, c2w, device, uid=i), params)
                yield out["render"], c2w

        image, uv, stats = texture_mesh(vertices, faces, colors, cam, views(), texel=texture_texel,
                                        tolerance=float(vol.voxel if texture_tolerance is None else texture_tolerance),
                                        max_level=int(texture_max_level))
        torch.cuda.synchronize(device)
        report.update({"texture_texel": texture_texel, "texture_size": stats["size"], "texture_fill": stats["fill"],
                       "texture_seen_share": stats["seen_share"], "texture_views": stats["views"],
                       "texture_faces_capped": stats["faces_capped"], "texture_s": time.perf_counter() - t0})
        result += ({"image": image, "uv": uv, "stats": stats},)
    return result
