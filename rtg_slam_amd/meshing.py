"""A triangle mesh of the map: TSDF fusion and marching tetrahedra on the HIP kernels of include/rtgs_slam.h, "meshing"
(csrc/tsdf.hip).  The reference has no mesher; this is the step the Gaussian-SLAM literature scores against the GT mesh:
depth rendered from the map (or the sensor's own), fused into a truncated signed distance volume, the zero level extracted.

    TsdfVolume        a dense axis-aligned grid (tsdf, weight, rgb planes, float32, x fastest) with integrate / extract_mesh
    mesh_from_map     walk a trajectory, fuse every `every`-th frame's rendered or sensor depth and colour, extract the mesh

The per-voxel rule and the extraction are restated in numpy in tests/tsdf_reference.py, which the kernels match bit for bit.
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
        for t in (depth, color):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError("rtg_slam_amd.meshing: tensors must live on a HIP device; this build has no CPU path.")
        if color.dim() != 3 or color.shape[0] != 3:
            raise ValueError("rtg_slam_amd.meshing: color must be [3,H,W]")
        H, W = int(color.shape[1]), int(color.shape[2])
        if depth.numel() != H * W:
            raise ValueError(f"rtg_slam_amd.meshing: depth has {depth.numel()} values, expected {H * W} for a {H}x{W} frame")
        dev = self.device
        if depth.device != dev or color.device != dev:
            raise ValueError("rtg_slam_amd.meshing: the frame and the volume live on different devices")
        fx, fy, cx, cy = _intrinsics(K)
        w2c = np.linalg.inv(_host_pose(c2w)).astype(np.float32)
        m = (C.c_float * 12)(*w2c[:3, :3].reshape(-1).tolist(), *w2c[:3, 3].tolist())
        d = depth.detach().float().contiguous()
        c = color.detach().float().contiguous()
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
        uk, inv = torch.unique(keys, sorted=True, return_inverse=True)
        # any holder of a key serves: equal keys carry bit-identical positions and colours
        first = torch.empty(uk.shape[0], dtype=torch.int64, device=dev)
        first.scatter_(0, inv, torch.arange(inv.shape[0], dtype=torch.int64, device=dev))
        out = (pos[first], inv.reshape(-1, 3).to(torch.int32), col[first])
        return out + (uk,) if return_keys else out


def map_bounds(mapper, pad: float):
    """The bounding box of the map's Gaussian centres, padded by `pad` on every side -> (lo, hi)."""
    xyz = mapper.opt.gaussian_data("all")["xyz"].detach()
    if xyz.shape[0] == 0:
        raise ValueError("rtg_slam_amd.meshing: the map holds no Gaussians")
    lo, hi = xyz.min(0).values.cpu().tolist(), xyz.max(0).values.cpu().tolist()
    return [l - pad for l in lo], [h + pad for h in hi]


def mesh_from_map(mapper, cam, poses=None, stream: Optional[Iterable] = None, *, voxel: float = 0.01, depth_source: str = "render",
                  every: int = 1, bounds=None, trunc: Optional[float] = None, max_weight: float = 64, min_weight: float = 1,
                  args=None, device=None, max_bytes: int = MAX_BYTES):
    """Fuse a trajectory into a TsdfVolume and extract its mesh -> (vertices, faces, colors, report).

    depth_source "render": the map (mapper.global_params) rendered at every pose by the evaluation renderer - a Renderer whose
    opaque threshold is args.renderer_opaque_threshold_eval, as evaluate_sequence constructs it - under no_grad, so the
    rasterizer runs with its no-backward flag; the rendered `depth` and `render` are fused.  "sensor": the stream's own depth
    and colour.  `stream` yields (depth, colour [3,H,W], GT c2w) as run_sequence's does; frame i is placed at poses[i], or at
    its GT pose without poses; "render" needs poses or a stream, "sensor" a stream.  Every `every`-th frame is fused.
    bounds = (lo, hi); default: the box of the map's Gaussian centres padded by trunc.  report: voxel, trunc, dims, bounds,
    frames fused, V, F and the seconds spent rendering, integrating and extracting."""
    from .mapping import Frame
    from .render import Renderer
    if depth_source not in ("render", "sensor"):
        raise ValueError(f"rtg_slam_amd.meshing: depth_source must be 'render' or 'sensor', got {depth_source!r}")
    if depth_source == "sensor" and stream is None:
        raise ValueError("rtg_slam_amd.meshing: depth_source='sensor' needs the frame stream")
    if stream is None and poses is None:
        raise ValueError("rtg_slam_amd.meshing: need poses or a stream")
    every = max(1, int(every))
    trunc = 4 * float(voxel) if trunc is None else float(trunc)
    if device is None:
        device = mapper.device
    device = torch.device(device)
    lo, hi = map_bounds(mapper, trunc) if bounds is None else bounds
    vol = TsdfVolume(lo, hi, voxel, trunc, max_weight, device, max_bytes)
    renderer = None
    if depth_source == "render":
        args = mapper.args if args is None else args
        eval_args = SimpleNamespace(**vars(args))
        eval_args.renderer_opaque_threshold = float(getattr(args, "renderer_opaque_threshold_eval", 0.5))
        renderer = Renderer(eval_args)
    t_render = t_integrate = 0.0
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
    t0 = time.perf_counter()
    vertices, faces, colors = vol.extract_mesh(min_weight)
    torch.cuda.synchronize(device)
    t_extract = time.perf_counter() - t0
    report: Dict = {"voxel": vol.voxel, "trunc": vol.trunc, "dims": list(vol.dims), "bounds": [list(vol.lo), list(vol.hi)],
                    "depth_source": depth_source, "every": every, "frames_fused": vol.frames, "V": int(vertices.shape[0]),
                    "F": int(faces.shape[0]), "render_s": t_render, "integrate_s": t_integrate, "extract_s": t_extract}
    return vertices, faces, colors, report
