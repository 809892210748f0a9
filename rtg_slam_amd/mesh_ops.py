"""Mesh clean-up on the HIP kernels of include/rtgs_slam.h, "mesh operations" (csrc/mesh_ops.hip) and "mesh decimation"
(csrc/mesh_decimate.hip): what a raw marching-tetrahedra mesh needs before it is usable.  The reference has no mesher and
so none of this.

    vertex_normals            area-weighted per-vertex normals, towards free space
    component_labels          label[v] = the smallest vertex index joined to v through faces
    remove_small_components   drop the faces of components with fewer than min_faces faces, then the vertices nobody uses
    compact                   drop the vertices no face uses, by itself
    keep_faces                keep the faces a caller's mask names, then drop the vertices nobody uses
    simplify_clusters         vertex clustering on a grid of `cell` metres: one vertex per occupied cell
    decimate                  quadric-error half-edge collapse to a target face count (csrc/mesh_decimate.hip): vertices are
                              removed, never moved, so corners stay sharp and the result stays manifold
    MeshDistance              the exact distance from points to the nearest face, and that face (csrc/mesh_distance.hip)
    register_to_mesh          rigid point-to-plane ICP of points to a MeshDistance's surface (csrc/mesh_register.hip sums the
                              normal equations in a fixed order; tests/mesh_register_reference.py is the definition)

All take an indexed mesh on the device - vertices [V,3] float32, faces [F,3] int32, colours [V,3] float32 - from
TsdfVolume.extract_mesh, SparseTsdfVolume.extract_mesh or another of these.  Every result is unique and independent of
thread order: two runs are bit-equal, and tests/mesh_ops_reference.py (decimate: tests/mesh_decimate_reference.py, MeshDistance:
tests/mesh_distance_reference.py) restates each in numpy, matched bit for bit.  The kernels do the float work and the per-element decisions; the scans and stable
sorts between them are torch's.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib

_K = _lib.CONSTANTS                  # the limits below are the header's (include/rtgs_slam.h)
MAX_CELLS = _K["RTGS_MESH_MAX_CELLS"]          # cells per axis, so that a key fits int64
DECIMATE_MIN_VALENCE = _K["RTGS_MESH_DECIMATE_MIN_VALENCE"]
DECIMATE_MAX_VALENCE = _K["RTGS_MESH_DECIMATE_MAX_VALENCE"]
DECIMATE_MAX_ROUNDS = _K["RTGS_MESH_DECIMATE_MAX_ROUNDS"]
_DECIMATE_HASH = 2654435761          # h(u) = u * this mod 2^32: the tie-break between equal costs
DISTANCE_BLOCK = _K["RTGS_MESH_DISTANCE_BLOCK"]
DISTANCE_SUPER = _K["RTGS_MESH_DISTANCE_SUPER"]
DISTANCE_MAX_DIM = _K["RTGS_MESH_DISTANCE_MAX_DIM"]      # cells per axis
DISTANCE_MAX_COORD = float(2 ** 20)  # the largest |coordinate| of a vertex pair_d2 is finite for
DISTANCE_LARGE_MAX = 64              # cell boxes of more cells go to the wave path of csrc/mesh_distance.hip
DISTANCE_CELL_EDGES = 2.0            # the default cell in mean edge lengths ("mesh distance", has the measurement)
DISTANCE_MIN_CELL_SHARE = 512        # ... but not below the mesh's extent / this
DISTANCE_SORT = True                 # sort the queries by cell first (same section: 6 to 14 times faster)
REGISTER_OUT = _K["RTGS_MESH_REGISTER_OUT"]    # 21 of J J^T, 6 of J r, r r, d2, the count
REGISTER_MIN_INLIERS = 6             # fewer correspondences do not determine a rigid motion
REGISTER_STOP = 1e-6                 # radians and metres: an update below both ends register_to_mesh

_p, _stream = _lib.ptr0, _lib.stream


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


def _corner_lists(faces, V):
    """-> (order, start): the corner indices 3 f + k sorted stably by their vertex, and every vertex's first position."""
    corner_vertex = faces.reshape(-1)
    order = torch.sort(corner_vertex, stable=True).indices
    start = torch.zeros(V + 1, dtype=torch.int64, device=faces.device)
    if faces.shape[0]:
        torch.cumsum(torch.bincount(corner_vertex, minlength=V), 0, out=start[1:])
    return order, start


def _decimate_round(vertices, faces, V, quadrics, remap, target, max_error):
    """One round on the current faces -> (the faces after it, the collapses applied).  quadrics and remap are updated."""
    dev = vertices.device
    lib = _lib.load()
    s = _stream(dev)
    Fn = int(faces.shape[0])
    order, start = _corner_lists(faces, V)
    # 1. locks: the vertices of every edge that does not have exactly 2 faces
    keys = torch.empty(3 * Fn, dtype=torch.int64, device=dev)
    locked = torch.zeros(V, dtype=torch.int32, device=dev)
    prop = torch.empty(V, dtype=torch.int32, device=dev)
    cost = torch.empty(V, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_decimate_edge_keys(_p(faces), Fn, V, _p(keys), s), "rtgs_mesh_decimate_edge_keys")
        edges, counts = torch.unique_consecutive(torch.sort(keys).values, return_counts=True)
        _lib.check(lib.rtgs_mesh_decimate_locks(_p(edges), _p(counts), int(edges.shape[0]), V, _p(locked), s),
                   "rtgs_mesh_decimate_locks")
        # 2. every removable vertex proposes its cheapest valid neighbour
        _lib.check(lib.rtgs_mesh_decimate_propose(_p(vertices), _p(faces), V, Fn, _p(order), _p(start), _p(locked), _p(quadrics),
                                                  0.0 if max_error is None else max_error, _p(prop), _p(cost), s),
                   "rtgs_mesh_decimate_propose")
    who = torch.nonzero(prop >= 0).reshape(-1)
    if who.shape[0] == 0:
        return faces, 0
    # 3. rank by (cost, h(u), u): h and u in one key (h < 2^32, u < 2^31), then stably by the cost, whose bits order as it does
    # (a cost is >= 0 and never NaN)
    by_hash = torch.sort((((who * _DECIMATE_HASH) & 0xFFFFFFFF) << 31) | who).indices
    by_cost = torch.sort(cost[who].view(torch.int64)[by_hash], stable=True).indices
    ranked = who[by_hash[by_cost]].contiguous()
    # 4. the 2 k lowest ranks claim their closed neighbourhoods; who holds all its claims is selected, the first k are applied
    k = (Fn - target + 1) // 2
    P = min(2 * k, int(ranked.shape[0]))
    claim = torch.full((V,), 2 ** 31 - 1, dtype=torch.int32, device=dev)
    selected = torch.empty(P, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_decimate_claim(_p(faces), _p(order), _p(start), _p(ranked), _p(prop), P, _p(claim), s),
                   "rtgs_mesh_decimate_claim")
        _lib.check(lib.rtgs_mesh_decimate_select(_p(faces), _p(order), _p(start), _p(ranked), _p(prop), P, _p(claim), _p(selected), s),
                   "rtgs_mesh_decimate_select")
    applied = (selected * (torch.cumsum(selected, 0) <= k)).to(torch.int32)
    # 5. apply, re-index, drop the faces that lost a corner
    keep = torch.empty(Fn, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_decimate_apply(_p(ranked), _p(prop), _p(applied), P, _p(remap), _p(quadrics), s),
                   "rtgs_mesh_decimate_apply")
        _lib.check(lib.rtgs_mesh_decimate_reindex(_p(faces), Fn, _p(remap), _p(keep), s), "rtgs_mesh_decimate_reindex")
    n = int(applied.sum())
    f_off, n_f = _exclusive(keep)
    if Fn - n_f != 2 * n:
        raise RuntimeError(f"rtg_slam_amd.mesh_ops: decimate applied {n} collapses and lost {Fn - n_f} faces, not {2 * n}")
    out_f = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    if n_f:
        with torch.cuda.device(dev):
            _lib.check(lib.rtgs_mesh_compact_faces(_p(faces), Fn, _p(keep), _p(f_off), _p(remap), _p(out_f), s),
                       "rtgs_mesh_compact_faces")
    return out_f, n


def decimate(vertices: torch.Tensor, faces: torch.Tensor, colors: torch.Tensor, target_faces: int,
             max_error: Optional[float] = None):
    """Quadric-error decimation by HALF-EDGE collapse to target_faces faces -> (vertices, faces, colors, stats).  A collapse
    u -> v removes vertex u and moves nothing: the output vertices and colours are a subset of the input's in their order,
    the surviving faces keep their order and winding, re-indexed.  It runs in rounds on the current faces:
      1  a vertex on an edge that does not have exactly 2 faces (boundary, non-manifold) is locked: never removed, but a
         possible target; neither is a vertex with fewer than DECIMATE_MIN_VALENCE or more than DECIMATE_MAX_VALENCE faces
      2  every other vertex u proposes the neighbour v of smallest (cost, v) among those that keep the surface sound (N(u) and
         N(v) share exactly 2 vertices; no face of u flips or loses its area) and, with max_error (metres) given, have
         sqrt(cost / weight) <= max_error; cost = p_v^T (Q[u] + Q[v]) p_v with the area-weighted plane quadrics Q in float64
      3  proposals are ranked by (cost, u * 2654435761 mod 2^32, u); k = ceil((F_now - target_faces) / 2) are still needed,
         the 2 k first take part
      4  each claims the closed neighbourhoods of u and v with an atomic minimum of its rank; who holds all its claims is
         selected, so no two selected collapses touch; the k first are applied: Q[v] += Q[u], faces re-indexed
    until F <= target_faces, a round applies nothing or DECIMATE_MAX_ROUNDS rounds ran; then the unused vertices go.  Every
    collapse removes exactly 2 faces, so the result has target_faces or target_faces - 1 faces when enough valid collapses
    exist.  stats: "rounds", "collapses", "faces_removed", "vertices_removed", "target_reached".  F <= target_faces returns
    the mesh compacted and otherwise untouched.  tests/mesh_decimate_reference.py is the definition, matched bit for bit."""
    target = int(target_faces)
    if target < 0:
        raise ValueError(f"rtg_slam_amd.mesh_ops: decimate needs target_faces >= 0, got {target}")
    if max_error is not None:
        max_error = float(max_error)
        if not max_error > 0:
            raise ValueError(f"rtg_slam_amd.mesh_ops: decimate needs max_error > 0 (metres) or None, got {max_error}")
    vertices, faces, colors, V, F = _check(vertices, faces, colors)
    dev = vertices.device
    rounds = collapses = 0
    if F > target:
        quadrics = torch.empty(V, 11, dtype=torch.float64, device=dev)
        order, start = _corner_lists(faces, V)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().rtgs_mesh_decimate_quadrics(_p(vertices), _p(faces), V, F, _p(order), _p(start), _p(quadrics),
                                                               _stream(dev)), "rtgs_mesh_decimate_quadrics")
        remap = torch.arange(V, dtype=torch.int32, device=dev)
        while faces.shape[0] > target and rounds < DECIMATE_MAX_ROUNDS:
            faces, n = _decimate_round(vertices, faces, V, quadrics, remap, target, max_error)
            rounds += 1
            collapses += n
            if n == 0:
                break
    out_v, out_f, out_c = _compact(vertices, faces, colors, V, int(faces.shape[0]), None)
    stats = {"rounds": rounds, "collapses": collapses, "faces_removed": F - int(out_f.shape[0]),
             "vertices_removed": V - int(out_v.shape[0]), "target_reached": int(out_f.shape[0]) <= target}
    return out_v, out_f, out_c, stats


def clean_mesh(vertices, faces, colors, *, min_component_faces: int = 0, simplify_cell: float = 0.0, origin=None,
               normals: bool = False, decimate_faces: int = 0,
               decimate_max_error: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor], Dict]:
    """The order meshing.mesh_from_map applies: removal (min_component_faces > 0), simplification (simplify_cell > 0, on the
    grid anchored at `origin`), decimation (decimate_faces > 0: the target face count), normals of the final mesh ->
    (vertices, faces, colors, normals or None, the removal stats).  A decimation adds its own stats to them as
    "decimate_rounds", "decimate_collapses", "decimate_faces_removed", "decimate_vertices_removed" and
    "decimate_target_reached"."""
    stats: Dict = {}
    if min_component_faces > 0:
        vertices, faces, colors, stats = remove_small_components(vertices, faces, colors, min_component_faces)
    if simplify_cell > 0:
        vertices, faces, colors = simplify_clusters(vertices, faces, colors, simplify_cell, origin)
    if decimate_faces > 0:
        vertices, faces, colors, dstats = decimate(vertices, faces, colors, decimate_faces, decimate_max_error)
        stats = {**stats, **{"decimate_" + k: v for k, v in dstats.items()}}
    nrm = vertex_normals(vertices, faces) if normals else None
    return vertices, faces, colors, nrm, stats


class MeshDistance:
    """The exact distance from points to the surface of an indexed triangle mesh (include/rtgs_slam.h, "mesh distance"):

        md = MeshDistance(vertices, faces)
        d2, face = md.query(points)                      # [N] float32 squared distances, [N] int32 nearest faces
        d2, face, normals = md.query(points, normals=True)
        d2, face = md.query(points, max_distance=0.1)    # the nearest face within 10 cm, or (inf, -1)

    d2[i] is the minimum over ALL faces of the float32 point-to-triangle chain pair_d2, face[i] the lowest face index that
    attains it, (inf, -1) for a point with a non-finite coordinate: bit for bit the brute force of
    tests/mesh_distance_reference.py, whatever `cell` is.  The index behind it is a uniform grid of `cell` metres over the
    mesh's box (default: DISTANCE_CELL_EDGES mean edge lengths, at least the extent / DISTANCE_MIN_CELL_SHARE) with the
    faces of every cell, and two levels of 4^3 blocks above it; it is built here, once, and refused with a ValueError that names the
    size when an axis would take more than DISTANCE_MAX_DIM cells, the grid 2^31 or more, or the cell table and the entries
    more than max_bytes.  The face indices are checked against V and F == 0 raises ValueError, here, once.  `sort`: take the
    queries in the order of their cells (a torch sort; the results land at the points' own rows); `large_max`: the largest
    cell box one thread registers.  Both change the time only."""

    def __init__(self, vertices: torch.Tensor, faces: torch.Tensor, cell: Optional[float] = None, max_bytes: int = 4 << 30,
                 large_max: Optional[int] = None, sort: Optional[bool] = None):
        self.vertices, self.faces, _, V, F = _check(vertices, faces)
        if F == 0:
            raise ValueError("rtg_slam_amd.mesh_ops: MeshDistance needs at least one face")
        if F >= 2 ** 31:
            raise ValueError(f"rtg_slam_amd.mesh_ops: {F} faces do not fit the int32 face index")
        dev = self.device = self.vertices.device
        self.sort = DISTANCE_SORT if sort is None else bool(sort)
        self.large_max = DISTANCE_LARGE_MAX if large_max is None else int(large_max)
        if not 0 <= self.large_max < 2 ** 31:
            raise ValueError(f"rtg_slam_amd.mesh_ops: large_max must lie in 0..2^31 - 1, got {large_max}")
        # one host read: the box, the largest |coordinate|, the mean edge length
        used = self.vertices[self.faces.reshape(-1).long()].reshape(F, 3, 3)
        edge = (used - used.roll(-1, 1)).double().norm(dim=2).mean()
        box = torch.cat([used.amin((0, 1)).double(), used.amax((0, 1)).double(), used.abs().amax().double().reshape(1),
                         edge.reshape(1)]).cpu().numpy()
        lo, hi, vmax, mean_edge = box[:3], box[3:6], float(box[6]), float(box[7])
        self.box = (lo.copy(), hi.copy())                                         # of the vertices the faces use, float64
        if not vmax <= DISTANCE_MAX_COORD:                                        # NaN fails too
            raise ValueError(f"rtg_slam_amd.mesh_ops: MeshDistance needs finite vertices with |coordinate| <= 2^20, found {vmax}")
        extent = float((hi - lo).max())
        if cell is None:
            cell = max(DISTANCE_CELL_EDGES * mean_edge, extent / DISTANCE_MIN_CELL_SHARE)
            cell = cell if cell > 0 else 1.0                                      # a mesh that is one point
        cell = float(np.float32(cell))
        if not 0 < cell < float("inf"):
            raise ValueError(f"rtg_slam_amd.mesh_ops: MeshDistance needs a finite cell > 0, got {cell}")
        origin = (lo - 0.75 * cell).astype(np.float32)                            # the kernels need half a cell of room
        dims = np.floor((hi - origin.astype(np.float64)) / cell).astype(np.int64) + 2
        size = f"{int(dims[0])} x {int(dims[1])} x {int(dims[2])} cells of {cell:g} m"
        if (dims > DISTANCE_MAX_DIM).any():
            raise ValueError(f"rtg_slam_amd.mesh_ops: MeshDistance would need {size}, more than {DISTANCE_MAX_DIM} on an axis; use a larger cell")
        if not ((lo - origin >= 0.5 * cell).all() and ((hi - origin) / cell + 0.5 <= dims).all()):
            raise ValueError(f"rtg_slam_amd.mesh_ops: a cell of {cell:g} m is below what float32 resolves at coordinates of {vmax:g}")
        cells = int(dims[0]) * int(dims[1]) * int(dims[2])
        bdims = (dims + DISTANCE_BLOCK - 1) // DISTANCE_BLOCK
        nblocks = int(np.prod(bdims)) + int(np.prod((bdims + DISTANCE_SUPER - 1) // DISTANCE_SUPER))      # and the super blocks
        table = 4 * (cells + 1) + nblocks
        if cells >= 2 ** 31:
            raise ValueError(f"rtg_slam_amd.mesh_ops: MeshDistance would need {size} = {cells} cells, the limit is 2^31 - 1; use a larger cell")
        if table > max_bytes:
            raise ValueError(f"rtg_slam_amd.mesh_ops: MeshDistance would need {size}: a cell table of {table} bytes "
                             f"({table / 2 ** 30:.2f} GiB), more than max_bytes = {int(max_bytes)}; use a larger cell")
        self.cell, self.dims, self.vmax = cell, tuple(int(d) for d in dims), float(np.float32(vmax))
        self._origin = (C.c_float * 3)(*origin.tolist())
        self._dims = (C.c_int32 * 3)(*self.dims)
        self.origin = tuple(float(x) for x in origin)
        lib = _lib.load()
        with torch.cuda.device(dev):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            counts = torch.zeros(cells, dtype=torch.int32, device=dev)
            self._queue = torch.zeros((lib.rtgs_mesh_distance_queue_bytes(F) + 3) // 4, dtype=torch.int32, device=dev)
            _lib.check(lib.rtgs_mesh_distance_count(_p(self.vertices), V, _p(self.faces), F, self._origin, cell, self._dims, self.vmax,
                                                    self.large_max, _p(counts), _p(self._queue), _stream(dev)), "rtgs_mesh_distance_count")
            incl = torch.cumsum(counts, 0, dtype=torch.int64)
            entries = int(incl[-1])                                               # the host read of the build
            total = table + 4 * entries
            if entries >= 2 ** 31 or total > max_bytes:
                raise ValueError(f"rtg_slam_amd.mesh_ops: MeshDistance would need {size} with {entries} entries: {total} bytes "
                                 f"({total / 2 ** 30:.2f} GiB), more than max_bytes = {int(max_bytes)} (or 2^31 entries); use a larger cell")
            self._start = torch.zeros(cells + 1, dtype=torch.int32, device=dev)
            self._start[1:] = incl
            del incl
            counts.zero_()                                                        # the cursors of the fill
            self._entries = torch.zeros(max(entries, 1), dtype=torch.int32, device=dev)       # every slot is a valid face index
            self._occupied = torch.empty(nblocks, dtype=torch.uint8, device=dev)
            _lib.check(lib.rtgs_mesh_distance_fill(_p(self.vertices), V, _p(self.faces), F, self._origin, cell, self._dims, self.vmax,
                                                   self.large_max, _p(self._start), _p(counts), _p(self._entries), _p(self._queue),
                                                   _stream(dev)), "rtgs_mesh_distance_fill")
            _lib.check(lib.rtgs_mesh_distance_blocks(_p(self._start), self._origin, cell, self._dims, _p(self._occupied), _stream(dev)),
                       "rtgs_mesh_distance_blocks")
            b.record()
        self._build = (a, b)
        self.entries, self.bytes = entries, total
        self.queries = 0
        self._events: List = []
        self._seconds = 0.0

    def _points(self, points):
        if not torch.is_tensor(points) or not points.is_cuda:
            raise RuntimeError("rtg_slam_amd.mesh_ops: tensors must live on a HIP device; this build has no CPU path.")
        if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
            raise ValueError("rtg_slam_amd.mesh_ops: points must be [N,3] float32")
        if points.device != self.device:
            raise ValueError("rtg_slam_amd.mesh_ops: the points and the mesh live on different devices")
        return points.detach().contiguous()

    def query(self, points: torch.Tensor, normals: bool = False, max_distance: Optional[float] = None):
        """-> (d2 [N] float32, face [N] int32), with normals=True also the unit normals [N,3] float32 of the hit faces
        (face_normals): new tensors, no synchronisation.  points [N,3] float32 on the mesh's device, anywhere in space.
        max_distance (metres, > 0): "the nearest face within it, or nothing" - a row stays what it is without the bound when
        its d2 <= max_d2 = float32(max_distance)^2 rounded to float32 (equality keeps it) and is (inf, -1), with the normal
        (0, 0, 0), otherwise (rtgs_mesh_distance_query_bounded; tests/mesh_distance_bounded_reference.py).  A point far from
        every face then costs a look at the super blocks around it, not its exact nearest face."""
        points = self._points(points)
        max_d2 = None
        if max_distance is not None:
            md = np.float32(max_distance)
            if not md > 0:                                                        # NaN too
                raise ValueError(f"rtg_slam_amd.mesh_ops: max_distance must be a number > 0 or None, got {max_distance}")
            with np.errstate(over="ignore"):
                max_d2 = float(md * md)                                           # float32; inf for a huge bound: unbounded
        dev, lib = self.device, _lib.load()
        N, V, F = int(points.shape[0]), int(self.vertices.shape[0]), int(self.faces.shape[0])
        d2 = torch.empty(N, dtype=torch.float32, device=dev)
        face = torch.empty(N, dtype=torch.int32, device=dev)
        if N:
            with torch.cuda.device(dev):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                order = None
                if self.sort:
                    keys = torch.empty(N, dtype=torch.int64, device=dev)
                    _lib.check(lib.rtgs_mesh_distance_keys(_p(points), N, self._origin, self.cell, self._dims, _p(keys), _stream(dev)),
                               "rtgs_mesh_distance_keys")
                    order = torch.sort(keys).indices.contiguous()
                if max_d2 is None:
                    _lib.check(lib.rtgs_mesh_distance_query(_p(points), N, _p(order), _p(self.vertices), V, _p(self.faces), F, self._origin,
                                                            self.cell, self._dims, self.vmax, _p(self._start), _p(self._entries),
                                                            _p(self._occupied), _p(d2), _p(face), _stream(dev)), "rtgs_mesh_distance_query")
                else:
                    _lib.check(lib.rtgs_mesh_distance_query_bounded(_p(points), N, _p(order), _p(self.vertices), V, _p(self.faces), F,
                                                                    self._origin, self.cell, self._dims, self.vmax, _p(self._start),
                                                                    _p(self._entries), _p(self._occupied), max_d2, _p(d2), _p(face),
                                                                    _stream(dev)), "rtgs_mesh_distance_query_bounded")
                b.record()
            self._events.append((a, b))
            self.queries += 1
        if not normals:
            return d2, face
        return d2, face, self.face_normals(face)

    def face_normals(self, face: torch.Tensor) -> torch.Tensor:
        """-> [N,3] float32: the unit normal (b - a) x (c - a) / l of face[i] ([N] int32 on the device), float32 in
        vertex_normals' order; (0, 0, 0) for a face without area and for face[i] < 0."""
        if not torch.is_tensor(face) or not face.is_cuda:
            raise RuntimeError("rtg_slam_amd.mesh_ops: tensors must live on a HIP device; this build has no CPU path.")
        if face.dim() != 1 or face.dtype != torch.int32 or face.device != self.device:
            raise ValueError("rtg_slam_amd.mesh_ops: face must be [N] int32 on the mesh's device")
        face = face.detach().contiguous()
        N = int(face.shape[0])
        out = torch.empty(N, 3, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().rtgs_mesh_distance_normals(_p(self.vertices), int(self.vertices.shape[0]), _p(self.faces),
                                                              int(self.faces.shape[0]), _p(face), N, _p(out), _stream(self.device)),
                       "rtgs_mesh_distance_normals")
        return out

    def report(self) -> Dict:
        """The grid and the device time of the build and of the queries so far (events; synchronises)."""
        for a, b in self._events:
            b.synchronize()
            self._seconds += a.elapsed_time(b) * 1e-3
        self._events = []
        self._build[1].synchronize()
        return {"cell": self.cell, "dims": list(self.dims), "cells": self.dims[0] * self.dims[1] * self.dims[2], "entries": self.entries,
                "bytes": self.bytes, "large_faces": int(self._queue[0]), "large_max": self.large_max, "sort": self.sort,
                "build_s": self._build[0].elapsed_time(self._build[1]) * 1e-3, "queries": self.queries, "query_s": self._seconds}


def face_unit_normals(vertices: torch.Tensor, faces: torch.Tensor, face: torch.Tensor) -> torch.Tensor:
    """MeshDistance.face_normals without the index: -> [N,3] float32, the unit normal of face[i] ([N] int32 on the device) of the
    mesh, (0, 0, 0) for a face without area and for face[i] < 0 (rtgs_mesh_distance_normals)."""
    vertices, faces, _, V, F = _check(vertices, faces)
    if F == 0:
        raise ValueError("rtg_slam_amd.mesh_ops: face_unit_normals needs at least one face")
    if not torch.is_tensor(face) or not face.is_cuda:
        raise RuntimeError("rtg_slam_amd.mesh_ops: tensors must live on a HIP device; this build has no CPU path.")
    if face.dim() != 1 or face.dtype != torch.int32 or face.device != vertices.device:
        raise ValueError("rtg_slam_amd.mesh_ops: face must be [N] int32 on the mesh's device")
    face = face.detach().contiguous()
    N = int(face.shape[0])
    out = torch.empty(N, 3, dtype=torch.float32, device=vertices.device)
    with torch.cuda.device(vertices.device):
        _lib.check(_lib.load().rtgs_mesh_distance_normals(_p(vertices), V, _p(faces), F, _p(face), N, _p(out), _stream(vertices.device)),
                   "rtgs_mesh_distance_normals")
    return out


def register_accumulate(points: torch.Tensor, face: torch.Tensor, d2: torch.Tensor, target: MeshDistance, center, max_d2: float,
                        source_normals: Optional[torch.Tensor] = None, min_cos: float = 0.0) -> torch.Tensor:
    """rtgs_mesh_register_accumulate -> out [30] float64 on the device, no synchronisation: the point-to-plane normal equations
    of points [N,3] float32 against the faces target.query gave them (face [N] int32, d2 [N] float32), summed in the fixed order
    of include/rtgs_slam.h, "mesh registration".  center: 3 numbers, rounded to float32; max_d2 and min_cos likewise."""
    points = target._points(points)
    N, dev = int(points.shape[0]), target.device
    for name, t, shape, dt in (("face", face, (N,), torch.int32), ("d2", d2, (N,), torch.float32),
                               ("source_normals", source_normals, (N, 3), torch.float32)):
        if t is None and name == "source_normals":
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("rtg_slam_amd.mesh_ops: tensors must live on a HIP device; this build has no CPU path.")
        if tuple(t.shape) != shape or t.dtype != dt or t.device != dev:
            raise ValueError(f"rtg_slam_amd.mesh_ops: {name} must be {list(shape)} {str(dt).split('.')[-1]} on the mesh's device")
    if N >= 2 ** 31:
        raise ValueError(f"rtg_slam_amd.mesh_ops: {N} points are more than the 2^31 - 1 one accumulation takes")
    face, d2 = face.detach().contiguous(), d2.detach().contiguous()
    sn = None if source_normals is None else source_normals.detach().contiguous()
    c = (C.c_float * 3)(*[float(np.float32(x)) for x in center])
    lib = _lib.load()
    scratch = torch.empty(max(lib.rtgs_mesh_register_scratch_bytes(N) // 8, 1), dtype=torch.float64, device=dev)
    out = torch.empty(REGISTER_OUT, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtgs_mesh_register_accumulate(_p(points), _p(face), _p(d2), _p(sn), N, _p(target.vertices),
                                                     int(target.vertices.shape[0]), _p(target.faces), int(target.faces.shape[0]), c,
                                                     float(np.float32(max_d2)), float(np.float32(min_cos)), _p(scratch), _p(out),
                                                     _stream(dev)), "rtgs_mesh_register_accumulate")
    return out


def _rodrigues(w):
    theta = np.sqrt(np.dot(w, w))
    if not theta > 0:
        return np.eye(3)
    k = w / theta
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def _register_solve(out, rank_tol):
    """The 30 sums -> (x, rank): A x = -b on the eigen-directions of A with lambda > rank_tol lambda_max."""
    A = np.zeros((6, 6), np.float64)
    A[np.triu_indices(6)] = out[:21]
    A = A + np.triu(A, 1).T
    b = np.asarray(out[21:27], dtype=np.float64)
    lam, vec = np.linalg.eigh(A)
    x, rank = np.zeros(6, np.float64), 0
    for j in range(6):
        if lam[j] > rank_tol * lam[5]:
            x = x - vec[:, j] * (np.dot(vec[:, j], b) / lam[j])
            rank += 1
    return x, rank


def register_to_mesh(points: torch.Tensor, target: MeshDistance, *, max_distance: float = 0.10, max_iterations: int = 30,
                     source_normals: Optional[torch.Tensor] = None, min_cos: float = 0.0, init=None,
                     rank_tol: float = 1e-8, bounded_query: bool = True) -> Tuple[np.ndarray, Dict]:
    """Rigid point-to-plane ICP of points [N,3] float32 (on the target's device) to the surface of `target` -> (T [4,4] float64
    on the host with T p near the surface, report).  T starts at `init` (4x4) or the identity and stays float64 on the host.
    Every iteration moves the ORIGINAL points by float32(T) (slam_ops.transform_map; source_normals [N,3] float32, if given,
    by its rotation), queries their nearest faces, sums the normal equations of the correspondences that take part
    (register_accumulate: d2 <= float32(max_distance)^2, a face with area, |n_source . n_face| >= min_cos) about the centre c
    of the target's vertex box, reads the 30 sums - the iteration's one host read - and solves A x = -b through
    numpy.linalg.eigh without the eigen-directions with lambda <= rank_tol lambda_max: what the geometry does not constrain
    stays put.  bounded_query: the iteration's query is target.query(moved, max_distance=max_distance) - the accumulation's
    own float32 gate - so that only the inliers pay for their nearest face; the rows it drops are the rows the gate drops, so
    T, the iterations and all 30 sums are bit for bit those of bounded_query=False.  x = (w, v) is applied as
    T <- Trans(c) [R(w) | v] Trans(-c) T, R the Rodrigues rotation.  It stops after an
    update with |w| <= 1e-6 rad and |v| <= 1e-6 m ("converged"), after max_iterations updates ("max iterations"), or, without
    an update, when fewer than 6 correspondences take part ("too few inliers").
    report: iterations (updates applied), converged, reason, inliers (per accumulation), inlier_share (the last / N),
    rms_plane_before / _after and rms_distance_before / _after (metres, of the first and the last accumulation: the plane
    residuals r and the query's distances over the inliers), rank (of the last solve), rotation_deg and translation_m (of
    T inverse(init): its angle, and how far it moves c), query_s and accumulate_s (device events, summed over the
    accumulations).  tests/mesh_register_reference.py is the definition: every device step is matched bit for bit and the host
    steps are the same float64 numpy operations."""
    from . import slam_ops as so
    if not isinstance(target, MeshDistance):
        raise ValueError("rtg_slam_amd.mesh_ops: register_to_mesh needs a MeshDistance as its target")
    points = target._points(points)
    N, dev = int(points.shape[0]), target.device
    if source_normals is not None:
        if not torch.is_tensor(source_normals) or not source_normals.is_cuda:
            raise RuntimeError("rtg_slam_amd.mesh_ops: tensors must live on a HIP device; this build has no CPU path.")
        if tuple(source_normals.shape) != (N, 3) or source_normals.dtype != torch.float32 or source_normals.device != dev:
            raise ValueError("rtg_slam_amd.mesh_ops: source_normals must be [N,3] float32, one row per point, on the mesh's device")
        source_normals = source_normals.detach().contiguous()
    max_iterations = int(max_iterations)
    if not float(max_distance) > 0 or max_iterations < 1:
        raise ValueError(f"rtg_slam_amd.mesh_ops: register_to_mesh needs max_distance > 0 and max_iterations >= 1, got "
                         f"{max_distance} and {max_iterations}")
    T0 = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    if T0.shape != (4, 4) or not np.isfinite(T0).all():
        raise ValueError("rtg_slam_amd.mesh_ops: init must be a finite 4x4 matrix")
    md = np.float32(max_distance)
    max_d2 = md * md                                                              # float32
    center = ((target.box[0] + target.box[1]) * 0.5).astype(np.float32)
    c = center.astype(np.float64)
    T = T0.copy()
    rep: Dict = {"iterations": 0, "converged": False, "reason": "max iterations", "inliers": [], "rank": 0}
    events: List = []
    first = last = None
    while True:
        T32 = T.astype(np.float32)
        with torch.cuda.device(dev):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            moved = so.transform_map(points, torch.from_numpy(T32))
            normals = None
            if source_normals is not None:
                R32 = T32.copy()
                R32[:3, 3] = 0.0
                normals = so.transform_map(source_normals, torch.from_numpy(R32))
            e[0].record()
            d2, face = target.query(moved, max_distance=max_distance if bounded_query else None)
            e[1].record()
            sums = register_accumulate(moved, face, d2, target, center, max_d2, normals, min_cos)
            e[2].record()
        events.append(e)
        out = sums.cpu().numpy()                                                  # the iteration's host read
        count = int(out[29])
        rep["inliers"].append(count)
        last = out
        first = out if first is None else first
        if count < REGISTER_MIN_INLIERS:
            rep["reason"] = "too few inliers"
            break
        x, rep["rank"] = _register_solve(out, rank_tol)
        D = np.eye(4)
        D[:3, :3] = _rodrigues(x[:3])
        D[:3, 3] = (c + x[3:]) - D[:3, :3] @ c
        T = D @ T
        rep["iterations"] += 1
        if np.sqrt(np.dot(x[:3], x[:3])) <= REGISTER_STOP and np.sqrt(np.dot(x[3:], x[3:])) <= REGISTER_STOP:
            rep["converged"], rep["reason"] = True, "converged"
            break
        if rep["iterations"] >= max_iterations:
            break
    for name, o in (("before", first), ("after", last)):
        n = o[29]
        rep["rms_plane_" + name] = float(np.sqrt(o[27] / n)) if n else float("nan")
        rep["rms_distance_" + name] = float(np.sqrt(o[28] / n)) if n else float("nan")
    rep["inlier_share"] = rep["inliers"][-1] / N if N else 0.0
    total = T @ np.linalg.inv(T0)
    rep["rotation_deg"] = float(np.degrees(np.arccos(np.clip(0.5 * (np.trace(total[:3, :3]) - 1.0), -1.0, 1.0))))
    rep["translation_m"] = float(np.linalg.norm(total[:3, :3] @ c + total[:3, 3] - c))
    events[-1][2].synchronize()
    rep["query_s"] = sum(e[0].elapsed_time(e[1]) for e in events) * 1e-3
    rep["accumulate_s"] = sum(e[1].elapsed_time(e[2]) for e in events) * 1e-3
    return T, rep
