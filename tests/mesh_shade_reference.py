"""Plain-numpy float32 restatement of the mesh renderer's colour pass (include/rtgs_slam.h, "mesh render", rtgs_mesh_shade;
evaluation.MeshRenderer.render_color), on top of tests/mesh_render_reference.py.  Used only by tests; it is the definition the
kernel shade_kernel of csrc/mesh_render.hip is held to, bit for bit.  Every float step is one correctly rounded float32
operation, in the order written here.

Per pixel     (px, py) with f = face_map[py][px].  The background when f < 0 or f >= F, or when the rasteriser's face setup fails
              for f at this view (a corner not usable, a u or v not finite, an empty box, two corners on one point): that cannot
              happen for a face map rendered at this pose, and must not fault for any other.
Weights       w0 = E(b, c), w1 = E(c, a), w2 = E(a, b) at ((float)px, (float)py): the very values whose signs admitted the
              pixel.  b0 = w0 iz_a, b1 = w1 iz_b, b2 = w2 iz_c, s = (b0 + b1) + b2, l_k = b_k / s: perspective-correct
              barycentrics.  The background when an l_k is not finite.
Vertex source c = (l0 c_a + l1 c_b) + l2 c_c per channel, then fmin(fmax(c, 0), 1).
Texture       tu = (l0 u_a + l1 u_b) + l2 u_c, tv likewise (uv [F,3,2], y down in 0..1).  X = fmin(fmax(tu Wt - 0.5, 0), Wt - 1)
              (a NaN gives 0), ix = floor(X), ix1 = min(ix + 1, Wt - 1), tx = X - ix; Y, iy, iy1, ty likewise with Ht.  A texel
              is byte / 255.  top = c00 + tx (c10 - c00), bot = c01 + tx (c11 - c01), c = top + ty (bot - top): the bake's
              bilinear form (mesh_texture_reference.bake_view)."""
import numpy as np

from tests import mesh_render_reference as rr

F32 = np.float32
NEAR = rr.NEAR


def weights(vertices, faces, face_map, K, H, W, c2w, near=NEAR):
    """-> (ok [H,W] bool, l [3,H,W] float32, face [H,W] int64, (w0, w1, w2) [H,W] float32): the pixels that get a colour, their
    perspective-correct barycentrics (garbage where not ok), the face index clamped into range, the edge values."""
    near = F32(near)
    assert near > 0
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    fm = np.ascontiguousarray(face_map, dtype=np.int32).reshape(H, W).astype(np.int64)
    F = len(f)
    ok = (fm >= 0) & (fm < F)
    if F == 0:
        z = np.zeros((H, W), F32)
        return ok, np.stack([z, z, z]), fm, (z, z, z)
    fi = np.where(ok, fm, 0)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px, py = xs.astype(F32), ys.astype(F32)
    with np.errstate(all="ignore"):
        u, v, iz, usable = rr.project(vertices, K, c2w, near)
        fu, fv, fiz = u[f], v[f], iz[f]                                   # [F,3]
        good = usable[f].all(axis=1) & np.isfinite(fu).all(axis=1) & np.isfinite(fv).all(axis=1)
        x0 = np.maximum(np.ceil(fu.min(axis=1)), F32(0))
        x1 = np.minimum(np.floor(fu.max(axis=1)), F32(W - 1))
        y0 = np.maximum(np.ceil(fv.min(axis=1)), F32(0))
        y1 = np.minimum(np.floor(fv.max(axis=1)), F32(H - 1))
        good &= (x0 <= x1) & (y0 <= y1)
        ok &= good[fi]
        au, av, bu, bv, cu, cv = fu[fi, 0], fv[fi, 0], fu[fi, 1], fv[fi, 1], fu[fi, 2], fv[fi, 2]
        w0, d0 = rr._edge(bu, bv, cu, cv, px, py)
        w1, d1 = rr._edge(cu, cv, au, av, px, py)
        w2, d2 = rr._edge(au, av, bu, bv, px, py)
        ok &= ~(d0 | d1 | d2)
        b0, b1, b2 = w0 * fiz[fi, 0], w1 * fiz[fi, 1], w2 * fiz[fi, 2]
        s = (b0 + b1) + b2
        l = np.stack([b0 / s, b1 / s, b2 / s])
        assert l.dtype == F32
        ok &= np.isfinite(l).all(axis=0)
    return ok, l, fi, (w0, w1, w2)


def shade(vertices, faces, face_map, K, H, W, c2w, colors=None, uv=None, texture=None, background=(0, 0, 0), near=NEAR):
    """-> [3,H,W] float32: the picture of the mesh whose face map (mesh_render_reference.render at c2w) is face_map, coloured
    from colors [V,3] float32 in 0..1, or from uv [F,3,2] float32 and texture [Ht,Wt,3] uint8."""
    if (colors is None) == (uv is None and texture is None) or (uv is None) != (texture is None):
        raise ValueError("shade: give colors, or uv and texture")
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    bg = np.asarray(background, dtype=F32).reshape(3)
    out = np.empty((3, H, W), dtype=F32)
    out[:] = bg[:, None, None]
    ok, l, fi, _ = weights(vertices, f, face_map, K, H, W, c2w, near)
    if not ok.any():
        return out
    l0, l1, l2 = l[0][ok], l[1][ok], l[2][ok]
    t = fi[ok]
    with np.errstate(all="ignore"):
        if colors is not None:
            c = np.ascontiguousarray(colors, dtype=F32).reshape(-1, 3)
            ca, cb, cc = c[f[t, 0]], c[f[t, 1]], c[f[t, 2]]                # [n,3]
            for k in range(3):
                val = (l0 * ca[:, k] + l1 * cb[:, k]) + l2 * cc[:, k]
                assert val.dtype == F32
                out[k][ok] = np.fmin(np.fmax(val, F32(0)), F32(1))
            return out
        q = np.ascontiguousarray(uv, dtype=F32).reshape(-1, 3, 2)[t]       # [n,3,2]
        tex = np.ascontiguousarray(texture)
        assert tex.dtype == np.uint8 and tex.ndim == 3 and tex.shape[2] == 3
        Ht, Wt = tex.shape[:2]
        tu = (l0 * q[:, 0, 0] + l1 * q[:, 1, 0]) + l2 * q[:, 2, 0]
        tv = (l0 * q[:, 0, 1] + l1 * q[:, 1, 1]) + l2 * q[:, 2, 1]
        X = np.fmin(np.fmax(tu * F32(Wt) - F32(0.5), F32(0)), F32(Wt - 1))
        Y = np.fmin(np.fmax(tv * F32(Ht) - F32(0.5), F32(0)), F32(Ht - 1))
        fx0, fy0 = np.floor(X), np.floor(Y)
        tx, ty = X - fx0, Y - fy0
        assert tx.dtype == F32 and ty.dtype == F32
        ix, iy = fx0.astype(np.int64), fy0.astype(np.int64)
        ix1, iy1 = np.minimum(ix + 1, Wt - 1), np.minimum(iy + 1, Ht - 1)
        for k in range(3):
            img = tex[..., k].astype(F32) / F32(255)
            c00, c10, c01, c11 = img[iy, ix], img[iy, ix1], img[iy1, ix], img[iy1, ix1]
            top = c00 + tx * (c10 - c00)
            bot = c01 + tx * (c11 - c01)
            val = top + ty * (bot - top)
            assert val.dtype == F32
            out[k][ok] = val
    return out
