"""Mesh clean-up on the HIP kernels of include/rtgs_slam.h, "mesh operations" (csrc/mesh_ops.hip): what a raw
marching-tetrahedra mesh needs before it is usable.  The reference has no mesher and so none of this.

    vertex_normals            area-weighted per-vertex normals, towards free space
    component_labels          label[v] = the smallest vertex index joined to v through faces
    remove_small_components   drop the faces of components with fewer than min_faces faces, then the vertices nobody uses
    compact                   drop the vertices no face uses, by itself
    keep_faces                keep the faces a caller's mask names, then drop the vertices nobody uses
    simplify_clusters         vertex clustering on a grid of `cell` metres: one vertex per occupied cell

All take an indexed mesh on the device - vertices [V,3] float32, faces [F,3] int32, colours [V,3] float32 - from
TsdfVolume.extract_mesh, SparseTsdfVolume.extract_mesh or another of these.  Every result is unique and independent of
thread order: two runs are bit-equal, and tests/mesh_ops_reference.py restates each in numpy, matched bit for bit.  The
kernels do the float work and the per-element decisions; the scans and stable sorts between them are torch's.
There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib

MAX_CELLS = 1 << 21                  # RTGS_MESH_MAX_CELLS: cells per axis, so that a key fits int64


def _p(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check(vertices, faces, colors=None):
    """The checks every operation shares -> (vertices, faces, colors) contiguous, V, F.  Face indices are checked against V
    here (one host synchronisation): the kernels trust them."""
    for t in (vertices, faces) + (() if colors is None else (colors,)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("rtg_slam_amd.mesh_ops: tensors must live on a HIP device; this build has no CPU path.")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError("rtg_slam_amd.mesh_ops: vertices must be [V,3] float32")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError("rtg_slam_amd.mesh_ops: faces must be [F,3] int32")
    if colors is not None and (colors.shape != vertices.shape or colors.dtype != torch.float32):
        raise ValueError("rtg_slam_amd.mesh_ops: colors must be [V,3] float32, one row per vertex")
    if faces.device != vertices.device or (colors is not None and colors.device != vertices.device):
        raise ValueError("rtg_slam_amd.mesh_ops: the mesh's tensors live on different devices")
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    _check_faces(faces, V)
    return (vertices.detach().contiguous(), faces.detach().contiguous(),
            None if colors is None else colors.detach().contiguous(), V, F)


def _check_faces(faces, V):
    if faces.shape[0]:
        lo, hi = (int(x) for x in torch.aminmax(faces))
        if lo < 0 or hi >= V:
            raise ValueError(f"rtg_slam_amd.mesh_ops: face indices must lie in 0..{V - 1}, found {lo}..{hi}")


def _exclusive(flags):
    """int32 flags -> (their exclusive scan as int64, their sum)."""
    if flags.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=flags.device), 0
    incl = torch.cumsum(flags, 0, dtype=torch.int64)
    return incl - flags, int(incl[-1])


def _run_starts(sorted_keys):
    """Sorted keys -> (the run index of every position, the starts of the runs with the total appended)."""
    _, inv, counts = torch.unique_consecutive(sorted_keys, return_inverse=True, return_counts=True)
    start = torch.zeros(counts.shape[0] + 1, dtype=torch.int64, device=sorted_keys.device)
    torch.cumsum(counts, 0, out=start[1:])
    return inv, start


def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """-> [V,3] float32: the normalised sum of the incident faces' area-weighted normals e1 x e2 (e1 = p1 - p0, e2 = p2 - p0;
    faces are wound towards free space, so the normals point there), every step one rounded float32 operation.  A vertex's
    sum starts at 0 and adds its corners in ascending corner index 3 f + k; it is divided by
    l = sqrt((x x + y y) + z z) when l > 0 and is (0, 0, 0) otherwise - an unreferenced vertex, or only area-less faces."""
    vertices, faces, _, V, F = _check(vertices, faces)
    dev = vertices.device
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    if V == 0:
        return out
    # the vertex-to-corner list: a stable sort keeps a vertex's corners in ascending corner index
    corner_vertex = faces.reshape(-1)
    order = torch.sort(corner_vertex, stable=True).indices
    start = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    if F:
        torch.cumsum(torch.bincount(corner_vertex, minlength=V), 0, out=start[1:])
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rtgs_mesh_vertex_normals(_p(vertices), _p(faces), V, F, _p(order), _p(start), _p(out), _stream(dev)),
                   "rtgs_mesh_vertex_normals")
    return out


def _labels(faces, V):
    dev = faces.device
    F = int(faces.shape[0])
    parent = torch.empty(V, dtype=torch.int32, device=dev)
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    if V:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().rtgs_mesh_component_labels(_p(faces), F, V, _p(parent), _p(labels), _stream(dev)),
                       "rtgs_mesh_component_labels")
    return labels


def component_labels(faces: torch.Tensor, V: int) -> torch.Tensor:
    """-> [V] int32: label[v] = the smallest vertex index among the vertices joined to v through faces (two vertices of one
    face are joined); an unreferenced vertex labels itself.  A lock-free union-find that only ever hooks a root under a
    smaller root, so the result does not depend on the order of the hooks."""
    if not torch.is_tensor(faces) or not faces.is_cuda:
        raise RuntimeError("rtg_slam_amd.mesh_ops: tensors must live on a HIP device; this build has no CPU path.")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError("rtg_slam_amd.mesh_ops: faces must be [F,3] int32")
    V = int(V)
    if V < 0:
        raise ValueError("rtg_slam_amd.mesh_ops: V must be >= 0")
    _check_faces(faces, V)
    return _labels(faces.detach().contiguous(), V)


def _compact(vertices, faces, colors, V, F, keep):
    """Faces with keep != 0 (None: all) in order, the vertices they use in order, faces re-indexed."""
    dev = vertices.device
    lib = _lib.load()
    used = torch.zeros(V, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_mark_vertices(_p(faces), F, _p(keep), _p(used), _stream(dev)), "rtgs_mesh_mark_vertices")
    v_off, n_v = _exclusive(used)
    f_off, n_f = (None, F) if keep is None else _exclusive(keep)
    out_v = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
    out_c = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    if n_v == 0:                         # no face survives: nothing to copy
        return out_v, out_f, out_c
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_compact_vertices(_p(vertices), _p(colors), V, _p(used), _p(v_off), _p(out_v), _p(out_c), _p(vmap),
                                                  _stream(dev)), "rtgs_mesh_compact_vertices")
        _lib.check(lib.rtgs_mesh_compact_faces(_p(faces), F, _p(keep), _p(f_off), _p(vmap), _p(out_f), _stream(dev)),
                   "rtgs_mesh_compact_faces")
    return out_v, out_f, out_c


def compact(vertices: torch.Tensor, faces: torch.Tensor, colors: torch.Tensor):
    """Drop the vertices no face references -> (vertices, faces, colors): the surviving vertices in their order, the faces
    in theirs, re-indexed."""
    vertices, faces, colors, V, F = _check(vertices, faces, colors)
    return _compact(vertices, faces, colors, V, F, None)


def keep_faces(vertices: torch.Tensor, faces: torch.Tensor, colors: Optional[torch.Tensor], keep: torch.Tensor):
    """The faces with keep != 0 (keep [F] int32 on the device, the caller's mask) in their order, the vertices they use in
    theirs, faces re-indexed -> (vertices, faces, colors).  colors may be None, and is then None in the result."""
    vertices, faces, colors, V, F = _check(vertices, faces, colors)
    if not torch.is_tensor(keep) or not keep.is_cuda:
        raise RuntimeError("rtg_slam_amd.mesh_ops: tensors must live on a HIP device; this build has no CPU path.")
    if keep.shape != (F,) or keep.dtype != torch.int32 or keep.device != vertices.device:
        raise ValueError("rtg_slam_amd.mesh_ops: keep must be [F] int32, one flag per face, on the mesh's device")
    keep = (keep.detach() != 0).to(torch.int32)           # the scan below sums the flags: 0 or 1
    # without colours the vertices stand in for them: the copy kernel moves both, the second result is dropped
    out_v, out_f, out_c = _compact(vertices, faces, vertices if colors is None else colors, V, F, keep)
    return out_v, out_f, None if colors is None else out_c


def remove_small_components(vertices: torch.Tensor, faces: torch.Tensor, colors: torch.Tensor, min_faces: int):
    """Drop the faces whose connected component (component_labels) has fewer than min_faces faces, then the vertices no
    surviving face references -> (vertices, faces, colors, stats).  Survivors keep their order; faces are re-indexed.
    stats: "components" (those with at least one face), "components_removed", "faces_removed", "vertices_removed"."""
    vertices, faces, colors, V, F = _check(vertices, faces, colors)
    min_faces = int(min_faces)
    if not -2 ** 31 <= min_faces < 2 ** 31:
        raise ValueError("rtg_slam_amd.mesh_ops: min_faces must fit int32")
    dev = vertices.device
    lib = _lib.load()
    labels = _labels(faces, V)
    counts = torch.zeros(V, dtype=torch.int32, device=dev)
    keep = torch.empty(F, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_component_faces(_p(faces), F, _p(labels), _p(counts), _stream(dev)), "rtgs_mesh_component_faces")
        _lib.check(lib.rtgs_mesh_keep_faces(_p(faces), F, _p(labels), _p(counts), min_faces, _p(keep), _stream(dev)),
                   "rtgs_mesh_keep_faces")
    out_v, out_f, out_c = _compact(vertices, faces, colors, V, F, keep)
    stats = {"components": int((counts > 0).sum()), "components_removed": int(((counts > 0) & (counts < min_faces)).sum()),
             "faces_removed": F - int(out_f.shape[0]), "vertices_removed": V - int(out_v.shape[0])}
    return out_v, out_f, out_c, stats


def simplify_clusters(vertices: torch.Tensor, faces: torch.Tensor, colors: torch.Tensor, cell: float, origin):
    """Vertex clustering -> (vertices, faces, colors).  A vertex's cell is (int) floor((p - origin) / cell) per axis in
    float32 (a vertex below origin raises ValueError), its key (cz ncy + cy) ncx + cx with nc one more than the largest index.
    One output vertex per occupied cell, in ascending key order: the mean position and colour of its members, added in
    float64 in ascending vertex index, divided by the count, rounded to float32.  Faces are re-indexed; a face with two
    corners in one cell is dropped, the others are rotated so that their smallest index comes first (winding kept), and of
    identical faces the first in original order stays (a mirrored duplicate is another face).  Survivors keep their order."""
    vertices, faces, colors, V, F = _check(vertices, faces, colors)
    cell = float(np.float32(cell))
    if not cell > 0:
        raise ValueError(f"rtg_slam_amd.mesh_ops: simplify_clusters needs cell > 0, got {cell}")
    origin = [float(np.float32(x)) for x in origin]
    if len(origin) != 3:
        raise ValueError("rtg_slam_amd.mesh_ops: origin must be 3 numbers")
    dev = vertices.device
    lib = _lib.load()
    empty_f = torch.zeros(0, 3, dtype=torch.int32, device=dev)
    if V == 0:
        return vertices.clone(), empty_f, colors.clone()
    cells = torch.empty(V, 3, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_cluster_cells(_p(vertices), V, (C.c_float * 3)(*origin), cell, _p(cells), _p(err), _stream(dev)),
                   "rtgs_mesh_cluster_cells")
    if int(err):
        raise ValueError(f"rtg_slam_amd.mesh_ops: a vertex lies below origin {origin} (or is not finite, or more than "
                         f"{MAX_CELLS} cells of {cell:g} m from it)")
    ncx, ncy, _ = (int(x) + 1 for x in cells.amax(0))
    keys = (cells[:, 2].to(torch.int64) * ncy + cells[:, 1]) * ncx + cells[:, 0]
    skeys, order = torch.sort(keys, stable=True)          # stable: a cell's members in ascending vertex index
    run, start = _run_starts(skeys)
    S = int(start.shape[0]) - 1
    cluster = torch.empty(V, dtype=torch.int32, device=dev)
    cluster[order] = run.to(torch.int32)
    out_v = torch.empty(S, 3, dtype=torch.float32, device=dev)
    out_c = torch.empty(S, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_cluster_means(_p(vertices), _p(colors), _p(order), _p(start), S, _p(out_v), _p(out_c),
                                               _stream(dev)), "rtgs_mesh_cluster_means")
    if F == 0:
        return out_v, empty_f, out_c
    mapped = torch.empty(F, 3, dtype=torch.int32, device=dev)
    valid = torch.empty(F, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_cluster_faces(_p(faces), F, _p(cluster), _p(mapped), _p(valid), _stream(dev)),
                   "rtgs_mesh_cluster_faces")
    # the valid faces sorted stably by (a, b, c): by (b, c) as one 64-bit key, then by a
    ids = torch.nonzero(valid).reshape(-1)
    m = mapped[ids].to(torch.int64)
    by_bc = torch.sort(m[:, 1] * S + m[:, 2], stable=True).indices
    by_a = torch.sort(m[by_bc, 0], stable=True).indices
    ids = ids[by_bc[by_a]].contiguous()
    keep = torch.zeros(F, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_mark_first(_p(mapped), _p(ids), int(ids.shape[0]), _p(keep), _stream(dev)), "rtgs_mesh_mark_first")
    f_off, n_f = _exclusive(keep)
    out_f = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    if n_f == 0:
        return out_v, out_f, out_c
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_compact_faces(_p(mapped), F, _p(keep), _p(f_off), _p(None), _p(out_f), _stream(dev)),
                   "rtgs_mesh_compact_faces")
    return out_v, out_f, out_c


def clean_mesh(vertices, faces, colors, *, min_component_faces: int = 0, simplify_cell: float = 0.0, origin=None,
               normals: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor], Dict]:
    """The order meshing.mesh_from_map applies: removal (min_component_faces > 0), simplification (simplify_cell > 0, on the
    grid anchored at `origin`), normals of the final mesh -> (vertices, faces, colors, normals or None, the removal stats)."""
    stats: Dict = {}
    if min_component_faces > 0:
        vertices, faces, colors, stats = remove_small_components(vertices, faces, colors, min_component_faces)
    if simplify_cell > 0:
        vertices, faces, colors = simplify_clusters(vertices, faces, colors, simplify_cell, origin)
    nrm = vertex_normals(vertices, faces) if normals else None
    return vertices, faces, colors, nrm, stats
