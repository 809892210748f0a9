"""On-disk formats of RTG-SLAM that sit either side of the hot path, readable / writable without
`plyfile` or `GPUtil`:

  * model snapshots  `iter_XXXX[_stable][_sibr|_merge].ply` - binary little-endian PLY, one `vertex` element, all
    float32, columns `x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity scale_0..2 rot_0..3 [confidence]`, RAW
    (pre-activation) values, SH stored channel-major (`_features_dc.transpose(1, 2).flatten()`):
    SLAM/gaussian_pointcloud.py:407-466 (writer), :118-193 (reader), SLAM/utils.py:321-392 (merge);
  * trajectories     `save_traj/pose_es.npy`, `pose_gt.npy` - float [n,4,4] camera-to-world: tracker.py:352-362;
  * `performance.json` - {"tracking", "mapping": mean seconds per frame, "fps": 1 / mapping, "gpu_memory": MB}:
    utils/monitor.py:22-50;
  * densified point clouds  `save_model/pcd_densify.ply` - binary little-endian PLY, one `vertex` element of float64
    `x y z nx ny nz`, the layout of Open3D's write_point_cloud (slam.py:146-150); read back as o3d.io.read_point_cloud
    reads it for eval_pcd (SLAM/eval.py:160), and model files likewise;
  * ground-truth meshes (PLY, ascii or binary little-endian; triangles and quads) and the surface sampling eval_pcd
    applies to them (trimesh.load / trimesh.sample.sample_surface, SLAM/eval.py:155-170), and the per-frame metrics
    table `statis_frame_*_iter_*.csv` with its mean row (metric.py:203-219, written there by pandas).

The packed [N,59] layout of rtg_slam_amd.map_optim (xyz | f_dc | f_rest coefficient-major | opacity | scaling |
rotation) converts to and from the file's columns here."""
from __future__ import annotations

import csv
import json
import math
import mmap
import os
from typing import Dict, List, Optional, Sequence

import numpy as np


def model_columns(include_confidence: bool = True, sh_rest: int = 45):
    cols = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(sh_rest)]
    cols += ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
    if include_confidence:
        cols.append("confidence")
    return cols


def _header(n: int, cols) -> bytes:
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    lines += [f"property float {c}" for c in cols] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def save_model_ply(path: str, xyz, features_dc, features_rest, opacity, scaling, rotation, confidence=None,
                   include_confidence: bool = True) -> None:
    """`GaussianPointCloud.save_model_ply` (gaussian_pointcloud.py:424-466).  features_dc [N,1,3], features_rest
    [N,15,3] (coefficient-major, as the model holds them); everything raw.  An empty cloud writes nothing, as there."""
    a = lambda t: np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)
    xyz = a(xyz).reshape(-1, 3)
    n = xyz.shape[0]
    if n == 0:
        return
    f_dc = a(features_dc).reshape(n, -1, 3).transpose(0, 2, 1).reshape(n, -1)          # channel-major on disk
    f_rest = a(features_rest).reshape(n, -1, 3).transpose(0, 2, 1).reshape(n, -1)
    cols = [xyz, np.zeros_like(xyz), f_dc, f_rest, a(opacity).reshape(n, 1), a(scaling).reshape(n, 3), a(rotation).reshape(n, 4)]
    if include_confidence:
        cols.append((np.zeros((n, 1), np.float32) if confidence is None else a(confidence).reshape(n, 1)))
    table = np.ascontiguousarray(np.concatenate(cols, axis=1).astype("<f4"))
    names = model_columns(include_confidence, f_rest.shape[1])
    assert table.shape[1] == len(names)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(_header(n, names))
        f.write(table.tobytes())


def _read_ply_table(path: str):
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt = f.readline().split()
        if fmt[:2] != [b"format", b"binary_little_endian"]:
            raise ValueError(f"{path}: only binary_little_endian PLY is supported, got {fmt}")
        n, names, in_vertex = 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated header")
            tok = line.split()
            if tok[:1] == [b"end_header"]:
                break
            if tok[:1] == [b"element"]:
                in_vertex = tok[1] == b"vertex"
                if in_vertex:
                    n = int(tok[2])
            elif tok[:1] == [b"property"] and in_vertex:
                if tok[1] not in (b"float", b"float32"):
                    raise ValueError(f"{path}: property {tok[2]!r} is {tok[1]!r}; RTG-SLAM models are all float32")
                names.append(tok[2].decode())
        table = np.frombuffer(f.read(n * len(names) * 4), dtype="<f4").reshape(n, len(names))
    return names, table


def load_model_ply(path: str, max_sh_degree: int = 3) -> Dict[str, np.ndarray]:
    """`GaussianPointCloud.load` (gaussian_pointcloud.py:118-193): columns are looked up BY NAME; `confidence` is
    optional (zeros if absent, e.g. the `_sibr` files).  Returns raw float32 arrays: xyz [N,3], features_dc [N,1,3],
    features_rest [N,15,3], opacity [N,1], scaling [N,3], rotation [N,4], confidence [N,1]."""
    names, t = _read_ply_table(path)
    col = {k: i for i, k in enumerate(names)}
    n = t.shape[0]
    pick = lambda prefix: sorted((k for k in names if k.startswith(prefix)), key=lambda k: int(k.split("_")[-1]))
    rest = pick("f_rest_")
    assert len(rest) == 3 * (max_sh_degree + 1) ** 2 - 3, (len(rest), max_sh_degree)
    f_dc = np.stack([t[:, col[f"f_dc_{i}"]] for i in range(3)], axis=1).reshape(n, 3, 1).transpose(0, 2, 1)
    f_rest = np.stack([t[:, col[k]] for k in rest], axis=1).reshape(n, 3, -1).transpose(0, 2, 1)
    conf = t[:, col["confidence"]].reshape(n, 1) if "confidence" in col else np.zeros((n, 1), np.float32)
    return dict(
        xyz=np.stack([t[:, col[k]] for k in ("x", "y", "z")], axis=1).copy(),
        features_dc=np.ascontiguousarray(f_dc), features_rest=np.ascontiguousarray(f_rest),
        opacity=t[:, col["opacity"]].reshape(n, 1).copy(),
        scaling=np.stack([t[:, col[k]] for k in pick("scale_")], axis=1).copy(),
        rotation=np.stack([t[:, col[k]] for k in pick("rot")], axis=1).copy(),
        confidence=conf.copy())


def merge_ply(path_a: str, path_b: str, path_out: str, include_confidence: bool = True) -> None:
    """SLAM/utils.py:321-392 `merge_ply`: the rows of two model files with the same columns, concatenated."""
    na, ta = _read_ply_table(path_a)
    nb, tb = _read_ply_table(path_b)
    want = model_columns(include_confidence, sum(k.startswith("f_rest_") for k in na))
    ia, ib = [na.index(k) for k in want], [nb.index(k) for k in want]
    table = np.ascontiguousarray(np.concatenate([ta[:, ia], tb[:, ib]], axis=0).astype("<f4"))
    with open(path_out, "wb") as f:
        f.write(_header(table.shape[0], want))
        f.write(table.tobytes())


def packed_to_model(packed) -> Dict[str, np.ndarray]:
    """map_optim's packed raw [N,59] -> the model's arrays (see module docstring for the column order)."""
    p = np.asarray(packed.detach().cpu().numpy() if hasattr(packed, "detach") else packed, dtype=np.float32)
    n = p.shape[0]
    return dict(xyz=p[:, 0:3], features_dc=p[:, 3:6].reshape(n, 1, 3), features_rest=p[:, 6:51].reshape(n, 15, 3),
                opacity=p[:, 51:52], scaling=p[:, 52:55], rotation=p[:, 55:59])


def model_to_packed(m: Dict[str, np.ndarray]) -> np.ndarray:
    n = m["xyz"].shape[0]
    return np.concatenate([m["xyz"], m["features_dc"].reshape(n, 3), m["features_rest"].reshape(n, 45), m["opacity"],
                           m["scaling"], m["rotation"]], axis=1).astype(np.float32)


def save_trajectories(save_path: str, pose_es, pose_gt=None) -> None:
    """tracker.py:352-362: `save_traj/pose_es.npy` (and `pose_gt.npy`), stacked [n,4,4] camera-to-world."""
    d = os.path.join(save_path, "save_traj")
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "pose_es.npy"), np.stack([np.asarray(p) for p in pose_es], axis=0))
    if pose_gt is not None:
        np.save(os.path.join(d, "pose_gt.npy"), np.stack([np.asarray(p) for p in pose_gt], axis=0))


class Recorder:
    """utils/monitor.py:10-50 without GPUtil: running means of per-frame seconds, fps = 1 / mean(mapping),
    peak GPU memory in MB (from torch.cuda instead of nvidia-smi), `performance.json`."""

    def __init__(self, gpu_id: int = 0) -> None:
        self._gpu_id = gpu_id
        self._value: Dict[str, float] = {}
        self._counter: Dict[str, int] = {}

    def update_max(self, name: str, value: float) -> None:
        if name not in self._value:
            self._value[name], self._counter[name] = value, 1
        else:
            self._value[name] = max(self._value[name], value)

    def update_mean(self, name: str, value: float, count: int) -> None:
        if count == 0:
            return
        if name not in self._value:
            self._value[name], self._counter[name] = value / count, count
        else:
            self._value[name] = (self._value[name] * self._counter[name] + value) / (self._counter[name] + count)
            self._counter[name] += count

    def cal_fps(self) -> None:
        self._value["fps"] = 1 / self._value["mapping"]
        self._counter["fps"] = 1

    def watch_gpu(self) -> float:
        import torch
        used = torch.cuda.max_memory_allocated(self._gpu_id) / (1024.0 * 1024.0) if torch.cuda.is_available() else 0.0
        self.update_max("gpu_memory", used)
        return used / 1024.0

    def save(self, directory: str) -> None:
        os.makedirs(directory, exist_ok=True)
        with open(os.path.join(directory, "performance.json"), "w") as f:
            json.dump(self._value, f)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _ply_header(f, path):
    if f.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, elements = None, []                    # elements: [name, count, [(prop, type) | (prop, (count_type, item_type))]]
    while True:
        line = f.readline()
        if not line:
            raise ValueError(f"{path}: truncated header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "end_header":
            break
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if tok[1] == "list":
                elements[-1][2].append((tok[4], (_PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]])))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii, binary_little_endian)")
    return fmt, elements


def _ply_binary_element(buf, pos, count, props):
    """One element's rows from a binary little-endian body -> ({prop: array or list of arrays}, new position)."""
    lists = [i for i, (_, t) in enumerate(props) if isinstance(t, tuple)]
    if not lists:
        dt = np.dtype([(n, "<" + t) for n, t in props])
        rows = np.frombuffer(buf, dtype=dt, count=count, offset=pos)
        return {n: rows[n] for n, _ in props}, pos + count * dt.itemsize
    if count == 0:
        return {n: np.zeros(0) for n, _ in props}, pos
    # fast path: every list of the element has the length its first row has (all triangles, or all quads)
    lens, p = [], pos
    for n, t in props:
        if isinstance(t, tuple):
            k = int(np.frombuffer(buf, dtype="<" + t[0], count=1, offset=p)[0])
            lens.append(k)
            p += np.dtype(t[0]).itemsize + k * np.dtype(t[1]).itemsize
        else:
            p += np.dtype(t).itemsize
    fields, li = [], 0
    for n, t in props:
        if isinstance(t, tuple):
            fields += [(n + "#n", "<" + t[0]), (n, "<" + t[1], (lens[li],))]
            li += 1
        else:
            fields.append((n, "<" + t))
    dt = np.dtype(fields)
    if pos + count * dt.itemsize <= len(buf):
        rows = np.frombuffer(buf, dtype=dt, count=count, offset=pos)
        li = 0
        ok = True
        for n, t in props:
            if isinstance(t, tuple):
                ok = ok and bool((rows[n + "#n"] == lens[li]).all())
                li += 1
        if ok:
            return {n: rows[n] for n, _ in props}, pos + count * dt.itemsize
    # mixed list lengths: row by row
    out = {n: [] for n, _ in props}
    for _ in range(count):
        for n, t in props:
            if isinstance(t, tuple):
                k = int(np.frombuffer(buf, dtype="<" + t[0], count=1, offset=pos)[0])
                pos += np.dtype(t[0]).itemsize
                out[n].append(np.frombuffer(buf, dtype="<" + t[1], count=k, offset=pos))
                pos += k * np.dtype(t[1]).itemsize
            else:
                out[n].append(np.frombuffer(buf, dtype="<" + t, count=1, offset=pos)[0])
                pos += np.dtype(t).itemsize
    return out, pos


def _ply_ascii_element(tokens, pos, count, props):
    if not any(isinstance(t, tuple) for _, t in props):
        m = len(props)
        block = np.asarray(tokens[pos:pos + count * m], dtype=np.float64).reshape(count, m)
        return {n: block[:, i] for i, (n, _) in enumerate(props)}, pos + count * m
    out = {n: [] for n, _ in props}
    for _ in range(count):
        for n, t in props:
            if isinstance(t, tuple):
                k = int(tokens[pos])
                out[n].append(np.asarray(tokens[pos + 1:pos + 1 + k], dtype=np.int64))
                pos += 1 + k
            else:
                out[n].append(float(tokens[pos]))
                pos += 1
    return out, pos


def _triangulate(polys) -> np.ndarray:
    """Face index lists -> [F,3] int64 triangles; a polygon (a, b, c, d, ...) becomes the fan (a,b,c), (a,c,d), ..."""
    if isinstance(polys, np.ndarray) and polys.ndim == 2:
        k = polys.shape[1]
        if k < 3:
            raise ValueError("PLY face with fewer than 3 vertices")
        fan = [np.stack([polys[:, 0], polys[:, j], polys[:, j + 1]], axis=1) for j in range(1, k - 1)]
        return np.stack(fan, axis=1).reshape(-1, 3).astype(np.int64)
    tris = []
    for p in polys:
        p = np.asarray(p, dtype=np.int64)
        if p.shape[0] < 3:
            raise ValueError("PLY face with fewer than 3 vertices")
        tris += [(p[0], p[j], p[j + 1]) for j in range(1, p.shape[0] - 1)]
    return np.asarray(tris, dtype=np.int64).reshape(-1, 3)


def load_mesh_ply(path: str, with_colors: bool = False):
    """A triangle mesh from a PLY file, ascii or binary little-endian (what trimesh.load reads for eval_pcd's GT mesh,
    SLAM/eval.py:155): -> (vertices float64 [V,3], faces int64 [F,3]).  Faces are lists of 3 or more vertex indices;
    quads (and larger polygons) are split into triangles (a,b,c), (a,c,d).  Other elements are skipped.  with_colors adds a
    third result: the vertices' red / green / blue as float64 [V,3] in 0..1 (uchar properties / 255), or None without them."""
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, path)
        body = f.read()
    verts, faces, colors = None, np.zeros((0, 3), np.int64), None
    if fmt == "ascii":
        tokens, pos = body.decode("ascii").split(), 0
        read = lambda count, props, pos: _ply_ascii_element(tokens, pos, count, props)
    else:
        pos = 0
        read = lambda count, props, pos: _ply_binary_element(body, pos, count, props)
    for name, count, props in elements:
        cols, pos = read(count, props, pos)
        if name == "vertex":
            verts = np.stack([np.asarray(cols[k], dtype=np.float64) for k in ("x", "y", "z")], axis=1)
            if all(k in cols for k in ("red", "green", "blue")):
                unit = 255.0 if dict(props)["red"] == "u1" else 1.0
                colors = np.stack([np.asarray(cols[k], dtype=np.float64) for k in ("red", "green", "blue")], axis=1) / unit
        elif name == "face":
            key = next((n for n, t in props if isinstance(t, tuple) and n in ("vertex_indices", "vertex_index")), None)
            if key is None:
                raise ValueError(f"{path}: face element without vertex_indices")
            faces = _triangulate(cols[key])
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    return (verts, faces, colors) if with_colors else (verts, faces)


def save_mesh_ply(path: str, vertices, faces, colors=None, normals=None) -> None:
    """An indexed triangle mesh as a binary little-endian PLY: float x y z (then float nx ny nz when normals [V,3] are given,
    then uchar red green blue when colors [V,3] in 0..1 are given, rounded to the nearest of 255 steps) per vertex,
    `list uchar int vertex_indices` per face.  Tensors or arrays; load_mesh_ply reads the file back with the vertices
    bit-equal (it skips the normals)."""
    to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    v = np.ascontiguousarray(to_np(vertices), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(to_np(faces)).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError(f"save_mesh_ply: face indices must lie in 0..{v.shape[0] - 1}")
    if v.shape[0] > 0x7fffffff:
        raise ValueError("save_mesh_ply: more vertices than an int index holds")
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    lines += [f"property float {c}" for c in "xyz"]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        nrm = np.ascontiguousarray(to_np(normals), dtype="<f4").reshape(-1, 3)
        if nrm.shape[0] != v.shape[0]:
            raise ValueError(f"save_mesh_ply: {nrm.shape[0]} normals for {v.shape[0]} vertices")
        lines += [f"property float {n}" for n in ("nx", "ny", "nz")]
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        c = to_np(colors).reshape(-1, 3)
        if c.shape[0] != v.shape[0]:
            raise ValueError(f"save_mesh_ply: {c.shape[0]} colours for {v.shape[0]} vertices")
        lines += [f"property uchar {n}" for n in ("red", "green", "blue")]
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    lines += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    vt = np.empty(v.shape[0], dtype=np.dtype(fields))
    vt["x"], vt["y"], vt["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        vt["nx"], vt["ny"], vt["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colors is not None:
        q = np.clip(np.rint(np.nan_to_num(c.astype(np.float64)) * 255.0), 0, 255).astype(np.uint8)
        vt["red"], vt["green"], vt["blue"] = q[:, 0], q[:, 1], q[:, 2]
    ft = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    ft["n"] = 3
    ft["i"] = f
    with open(path, "wb") as out:
        out.write(("\n".join(lines) + "\n").encode("ascii"))
        out.write(vt.tobytes())
        out.write(ft.tobytes())


def save_textured_obj(path: str, vertices, faces, uv, image, normals=None, image_name: Optional[str] = None) -> None:
    """A textured triangle mesh as Wavefront OBJ: `path` (X.obj), X.mtl beside it and the texture as a PNG (image_name, in
    the OBJ's directory; default X.png), written through PIL.  vertices [V,3], faces [F,3], uv [F,3,2] (three texture
    coordinates per face, x right and y DOWN in 0..1, as meshing.texture_mesh gives them), image [Ht,Wt,3] uint8, normals [V,3]
    or None.  The file holds `v` (and `vn`), three `vt` per face with v = 1 - y (OBJ's origin is the lower left corner), and
    `f a/ta b/tb c/tc` (`a/ta/a` with normals), under `mtllib` and `usemtl`.  Floats are written so that load_textured_obj
    returns equal arrays."""
    from PIL import Image
    to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    v = np.ascontiguousarray(to_np(vertices), dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(to_np(faces)).astype(np.int64).reshape(-1, 3)
    t = np.ascontiguousarray(to_np(uv), dtype=np.float32).reshape(-1, 3, 2)
    img = np.ascontiguousarray(to_np(image))
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError(f"save_textured_obj: face indices must lie in 0..{v.shape[0] - 1}")
    if t.shape[0] != f.shape[0]:
        raise ValueError(f"save_textured_obj: {t.shape[0]} rows of texture coordinates for {f.shape[0]} faces")
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("save_textured_obj: the image must be [Ht,Wt,3] uint8")
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    image_name = name + ".png" if image_name is None else image_name
    lines = [f"mtllib {name}.mtl", "usemtl textured"]
    lines += ["v %.9g %.9g %.9g" % tuple(r) for r in v.tolist()]
    if normals is not None:
        nrm = np.ascontiguousarray(to_np(normals), dtype=np.float32).reshape(-1, 3)
        if nrm.shape[0] != v.shape[0]:
            raise ValueError(f"save_textured_obj: {nrm.shape[0]} normals for {v.shape[0]} vertices")
        lines += ["vn %.9g %.9g %.9g" % tuple(r) for r in nrm.tolist()]
    t64 = t.astype(np.float64).reshape(-1, 2)
    lines += [f"vt {x!r} {1.0 - y!r}" for x, y in t64.tolist()]                  # 1 - y is exact in float64 for a float32 y >= 2^-29
    corner = "{0}/{1}/{0}" if normals is not None else "{0}/{1}"
    for i, (a, b, c) in enumerate((f + 1).tolist()):
        lines.append("f " + " ".join(corner.format(p, 3 * i + k + 1) for k, p in enumerate((a, b, c))))
    with open(path, "w") as out:
        out.write("\n".join(lines) + "\n")
    with open(stem + ".mtl", "w") as out:
        out.write(f"newmtl textured\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {image_name}\n")
    Image.fromarray(img).save(os.path.join(os.path.dirname(path), image_name))


def load_textured_obj(path: str):
    """What save_textured_obj wrote -> (vertices float32 [V,3], faces int32 [F,3], uv float32 [F,3,2] with y down, image uint8
    [Ht,Wt,3] from the material's map_Kd).  Triangles with `v/vt` or `v/vt/vn` corners only."""
    from PIL import Image
    v, vt, fv, ft, mtl = [], [], [], [], None
    with open(path) as src:
        for line in src:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                v.append([float(x) for x in w[1:4]])
            elif w[0] == "vt":
                vt.append((float(w[1]), 1.0 - float(w[2])))
            elif w[0] == "f":
                if len(w) != 4:
                    raise ValueError(f"{path}: only triangles are read, found a face of {len(w) - 1} corners")
                c = [p.split("/") for p in w[1:]]
                if any(len(p) < 2 or not p[1] for p in c):
                    raise ValueError(f"{path}: a face corner without a texture coordinate")
                fv.append([int(p[0]) - 1 for p in c])
                ft.append([int(p[1]) - 1 for p in c])
            elif w[0] == "mtllib":
                mtl = line.split(None, 1)[1].strip()
    if mtl is None:
        raise ValueError(f"{path}: no mtllib")
    base = os.path.dirname(path)
    tex = None
    with open(os.path.join(base, mtl)) as src:
        for line in src:
            if line.split()[:1] == ["map_Kd"]:
                tex = line.split(None, 1)[1].strip()
    if tex is None:
        raise ValueError(f"{os.path.join(base, mtl)}: no map_Kd")
    image = np.asarray(Image.open(os.path.join(base, tex)).convert("RGB"), dtype=np.uint8)
    vt = np.asarray(vt, dtype=np.float64).reshape(-1, 2)
    ft = np.asarray(ft, dtype=np.int64).reshape(-1, 3)
    return (np.asarray(v, dtype=np.float32).reshape(-1, 3), np.asarray(fv, dtype=np.int32).reshape(-1, 3),
            vt[ft].astype(np.float32).reshape(-1, 3, 2), image)


def sample_mesh_surface(vertices, faces, n: int, seed: int = 0):
    """n points uniformly on the surface (trimesh.sample.sample_surface, which eval_pcd applies to the GT mesh): a face with
    probability proportional to its area, then a uniform point of it (barycentric u, v in the unit square, folded into the
    triangle).  -> (points float64 [n,3], face index int64 [n])."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    if f.shape[0] == 0 or not area.sum() > 0:
        raise ValueError("sample_mesh_surface: the mesh has no area")
    rng = np.random.default_rng(seed)
    cum = np.cumsum(area)
    face = np.minimum(np.searchsorted(cum, rng.random(n) * cum[-1], side="right"), f.shape[0] - 1).astype(np.int64)
    uv = rng.random((n, 2))
    flip = uv.sum(axis=1) > 1.0
    uv[flip] = 1.0 - uv[flip]
    pts = a[face] + uv[:, :1] * (b[face] - a[face]) + uv[:, 1:] * (c[face] - a[face])
    return pts, face


POINT_CLOUD_COLUMNS = ("x", "y", "z", "nx", "ny", "nz")


def point_cloud_header(n: int) -> bytes:
    """The header Open3D's write_point_cloud gives a binary cloud with normals and no colours (as far as it is known
    without Open3D: not compared byte for byte against a file Open3D wrote)."""
    lines = ["ply", "format binary_little_endian 1.0", "comment Created by Open3D", f"element vertex {int(n)}"]
    lines += [f"property double {c}" for c in POINT_CLOUD_COLUMNS] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


class PointCloudPlyWriter:
    """Streams `n` float64 records (x y z nx ny nz) into a point-cloud PLY in pieces: the header first, then write(rows)
    with [m,6] float64 arrays (or anything exposing that buffer) until n rows are in.  close() checks the count."""

    def __init__(self, path: str, n: int):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.path, self.n, self.written = path, int(n), 0
        self._f = open(path, "wb")
        self._f.write(point_cloud_header(self.n))

    def write(self, rows) -> None:
        a = np.asarray(rows)
        if a.dtype != np.float64 or a.ndim != 2 or a.shape[1] != 6:
            raise ValueError("PointCloudPlyWriter.write: rows must be float64 [m, 6]")
        if self.written + a.shape[0] > self.n:
            raise ValueError(f"PointCloudPlyWriter.write: more than the {self.n} rows of the header")
        self._f.write(memoryview(np.ascontiguousarray(a)).cast("B"))
        self.written += a.shape[0]

    def close(self) -> None:
        if self._f is None:
            return
        self._f.close()
        self._f = None
        if self.written != self.n:
            raise ValueError(f"{self.path}: {self.written} rows written, the header says {self.n}")

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        elif self._f is not None:
            self._f.close()
            self._f = None


def save_point_cloud_ply(path: str, xyz, normals) -> int:
    """o3d.io.write_point_cloud of a cloud with normals: float64 records x y z nx ny nz.  An empty cloud writes no file (Open3D
    refuses to write one, we believe).  -> the number of points."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    if xyz.shape != nrm.shape:
        raise ValueError("save_point_cloud_ply: xyz and normals differ in shape")
    if xyz.shape[0] == 0:
        return 0
    with PointCloudPlyWriter(path, xyz.shape[0]) as w:
        w.write(np.concatenate([xyz, nrm], axis=1))
    return xyz.shape[0]


def load_point_cloud_ply(path: str):
    """o3d.io.read_point_cloud as eval_pcd uses it (SLAM/eval.py:160): the `vertex` element's x y z and, when all three are
    present, nx ny nz, as float or double in any property order, ascii or binary little-endian; other properties and elements
    are skipped.  A binary body is memory-mapped, not read into memory first.  -> (xyz float64 [N,3], normals float64 [N,3]
    or None).  Reads pcd_densify.ply and model files alike."""
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, path)
        pos = f.tell()
        if fmt == "ascii":
            tokens, pos = f.read().decode("ascii").split(), 0
            read = lambda count, props, pos: _ply_ascii_element(tokens, pos, count, props)
        else:
            buf = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
            read = lambda count, props, pos: _ply_binary_element(buf, pos, count, props)
    for name, count, props in elements:
        cols, pos = read(count, props, pos)
        if name != "vertex":
            continue
        names = [n for n, _ in props]
        if not all(c in names for c in ("x", "y", "z")):
            raise ValueError(f"{path}: vertex element without x, y, z")
        xyz = np.stack([np.asarray(cols[c], dtype=np.float64) for c in ("x", "y", "z")], axis=1)
        nrm = None
        if all(c in names for c in ("nx", "ny", "nz")):
            nrm = np.stack([np.asarray(cols[c], dtype=np.float64) for c in ("nx", "ny", "nz")], axis=1)
        return xyz, nrm                         # the copies above release the mapping
    raise ValueError(f"{path}: no vertex element")


def _is_number(x) -> bool:
    return isinstance(x, (int, float, np.integer, np.floating)) and not (isinstance(x, (float, np.floating)) and math.isnan(x))


def metrics_mean_row(rows: Sequence[Dict]) -> Dict:
    """metric.py:205-209's mean row: per column (in order of first appearance) the mean of its numeric values, NaN and
    missing cells skipped as pandas does; a column without numbers stays None; `frame` = "mean"."""
    cols: List[str] = []
    for r in rows:
        cols += [k for k in r if k not in cols]
    mean = {}
    for k in cols:
        vals = [float(r[k]) for r in rows if k in r and _is_number(r[k])]
        mean[k] = sum(vals) / len(vals) if vals else None
    mean["frame"] = "mean"
    return mean


def save_metrics_csv(path: str, rows: Sequence[Dict]) -> None:
    """metric.py:203-219 without pandas: one line per frame, then the mean row; the first column is the row index, as
    DataFrame.to_csv writes it.  NaN and None are empty cells."""
    rows = list(rows)
    table = rows + [metrics_mean_row(rows)]
    cols: List[str] = []
    for r in table:
        cols += [k for k in r if k not in cols]

    def cell(x):
        if x is None or (isinstance(x, (float, np.floating)) and math.isnan(x)):
            return ""
        if isinstance(x, (float, np.floating)):
            return repr(float(x))
        return str(x)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow([""] + cols)
        for i, r in enumerate(table):
            w.writerow([str(i)] + [cell(r.get(k)) for k in cols])
