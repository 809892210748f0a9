"""The hand-made scenes of the colour pass, shared by tests/test_mesh_shade_cpu.py (the definition against facts) and
tests/test_mesh_shade_gpu.py (the kernel against the definition), all at 64 x 48.

HAND is the identity camera with fx = fy = 64, cx = 32, cy = 24: a point made by at(u, v, z) with z a power of two projects to
(u, v) exactly, the edge values of a right triangle with legs of 32 pixels are integers and their sum is 1024, so every
barycentric is a multiple of 2^-10 and every blend of dyadic colours or texture coordinates is exact."""
import numpy as np

from rtg_slam_amd import synth
from tests import mesh_render_reference as rr
from tests import mesh_texture_reference as tr

F32 = np.float32
HAND = synth.CameraSpec(48, 64, 64.0, 64.0, 32.0, 24.0)
EYE = np.eye(4)
POISON = (255, 0, 255)                               # the colour of texels no fetch may touch


def K(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy)


def at(u, v, z):
    """The point that HAND at the identity projects to (u, v) at depth z."""
    return [(u - 32.0) * z / 64.0, (v - 24.0) * z / 64.0, z]


def face_map(case):
    """The case's own face map, or the definition's render of its mesh at its pose."""
    if case.get("face_map") is not None:
        return case["face_map"]
    cam = case["cam"]
    return rr.render(case["v"], case["f"], K(cam), cam.H, cam.W, case["c2w"])[1]


def _case(v, f, c2w=EYE, cam=HAND, **kw):
    return dict(v=np.asarray(v, F32).reshape(-1, 3), f=np.asarray(f, np.int32).reshape(-1, 3), c2w=np.asarray(c2w, np.float64),
                cam=cam, colors=None, uv=None, texture=None, face_map=None, background=(0.0, 0.0, 0.0)) | kw


# ---- a quad seen at 60 degrees from its normal: colours linear in the world position ----
RAMP_HALF = 1.5


def ramp_color(p):
    """[..., 3] world points -> [..., 3] colours, linear, inside 0.05 .. 0.95 on the quad."""
    p = np.asarray(p, dtype=np.float64)
    return np.stack([0.5 + 0.2 * p[..., 0] + 0.1 * p[..., 1], 0.5 - 0.1 * p[..., 0] + 0.2 * p[..., 1],
                     0.3 + 0.1 * p[..., 0] - 0.1 * p[..., 1]], -1)


def ramp_pose(angle_deg=60.0, distance=3.0):
    """A camera `distance` from the origin, looking at it, its axis at angle_deg from the normal (0, 0, 1) of the plane z = 0."""
    a = np.deg2rad(angle_deg)
    o = distance * np.array([np.sin(a), 0.0, -np.cos(a)])
    fwd = -o / np.linalg.norm(o)
    right = np.cross([0.0, 1.0, 0.0], fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, down, fwd, o
    return c2w


def ramp():
    h = RAMP_HALF
    v = np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], F32)
    uv = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], F32)
    texture = np.random.default_rng(7).integers(0, 256, (5, 7, 3)).astype(np.uint8)
    return _case(v, [[0, 1, 2], [0, 2, 3]], ramp_pose(), colors=ramp_color(v).astype(F32), uv=uv, texture=texture,
                 background=(0.25, 0.5, 0.75))


# ---- two triangles whose shared edge runs through pixel centres ----
QUAD = [at(8, 4, 2.0), at(40, 4, 2.0), at(40, 36, 2.0), at(8, 36, 2.0)]
PALETTE = np.array([[1.0, 0.25, 0.0], [0.0, 0.5, 1.0]], F32)         # face 0, face 1


def shared_edge(flip=False):
    """The quad (8, 4) .. (40, 36) at z = 2 split along the diagonal through (8 + k, 4 + k); every face has vertices of its own,
    all three in the face's palette colour, so a pixel shows which face shaded it."""
    v = [QUAD[0], QUAD[1], QUAD[2], QUAD[0], QUAD[2], QUAD[3]]
    f = [[0, 2, 1], [3, 5, 4]] if flip else [[0, 1, 2], [3, 4, 5]]
    return _case(v, f, colors=np.repeat(PALETTE, 3, axis=0))


def shared_edge_linear(flip=False):
    """The same two triangles on four shared vertices, coloured (u / 64, v / 64, 0.5): the picture is that function, exactly."""
    colors = np.array([[8 / 64, 4 / 64, 0.5], [40 / 64, 4 / 64, 0.5], [40 / 64, 36 / 64, 0.5], [8 / 64, 36 / 64, 0.5]], F32)
    return _case(QUAD, [[0, 2, 1], [0, 3, 2]] if flip else [[0, 1, 2], [0, 2, 3]], colors=colors)


# ---- the texture source ----
ATLAS_2X2 = np.array([[[10, 20, 30], [200, 100, 50]], [[0, 255, 128], [77, 1, 254]]], np.uint8)


def atlas_2x2(texture=ATLAS_2X2):
    """The quad with uv exactly 0 and 1 at its corners on a 2 x 2 atlas: X = 2 tu - 0.5 runs from -0.5 to 1.5 and is clamped at
    every border."""
    uv = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], F32)
    return _case(QUAD, [[0, 1, 2], [0, 2, 3]], uv=uv, texture=texture)


BLOCK_LEVELS = np.array([1, 3, 1, 2], np.int32)


def blocks(constant=None):
    """Four right triangles with legs of 32 pixels (at z = 1, 2, 2, 4) on the atlas mesh_texture_reference lays out for the levels
    1, 3, 1, 2.  Every block holds one colour of its own, every texel outside a block POISON; with `constant` the whole atlas
    holds that one colour."""
    corners = ((0, 2, 1.0), (30, 2, 2.0), (0, 14, 2.0), (30, 12, 4.0))
    v, f = [], []
    for k, (u, w, z) in enumerate(corners):
        v += [at(u, w, z), at(u + 32, w, z), at(u, w + 32, z)]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    lay = tr.layout(BLOCK_LEVELS)
    uv = tr.face_uv(lay, BLOCK_LEVELS)
    texture = np.empty((lay["Ht"], lay["Wt"], 3), np.uint8)
    texture[:] = POISON if constant is None else constant
    colours = np.array([[3, 60, 200], [250, 128, 1], [90, 90, 17], [33, 255, 64]], np.uint8)
    if constant is None:
        for k, (x0, y0) in enumerate(lay["origin"]):
            s = 1 << int(BLOCK_LEVELS[k])
            texture[y0:y0 + s, x0:x0 + s] = colours[k]
    return _case(v, f, uv=uv, texture=texture), colours


# ---- inputs that draw nothing ----
def nothing_cases():
    tri = [at(8, 4, 2.0), at(40, 4, 2.0), at(8, 36, 2.0)]
    colors = np.full((3, 3), 0.5, F32)
    bg = (0.125, 0.5, 0.875)
    zeros = np.zeros((HAND.H, HAND.W), np.int32)
    wild = np.random.default_rng(2).integers(-2 ** 31, 2 ** 31 - 1, (HAND.H, HAND.W)).astype(np.int32)
    wild[(wild >= 0) & (wild < 1)] = -1
    across = [[0.0, 0.0, -1.0]] + tri[1:]
    return {
        "a face map of -1": _case(tri, [[0, 1, 2]], colors=colors, face_map=zeros - 1, background=bg),
        "no faces": _case(tri, np.zeros((0, 3)), colors=colors, face_map=zeros, background=bg),
        "face indices out of range": _case(tri, [[0, 1, 2]], colors=colors, face_map=wild, background=bg),
        "a face across the near plane": _case(across, [[0, 1, 2]], colors=colors, face_map=zeros, background=bg),
        "a face with a NaN corner": _case([[np.nan, 0, 2]] + tri[1:], [[0, 1, 2]], colors=colors, face_map=zeros, background=bg),
        "a face of no area": _case([tri[0], tri[0], tri[1]], [[0, 1, 2]], colors=colors, face_map=zeros, background=bg),
    }


def hand_cases():
    """name -> case, every hand-made scene above."""
    cases = {"ramp": ramp(), "atlas 2x2": atlas_2x2(), "blocks": blocks()[0], "blocks constant": blocks((9, 99, 199))[0]}
    for flip in (False, True):
        cases[f"shared edge flip={flip}"] = shared_edge(flip)
        cases[f"shared edge linear flip={flip}"] = shared_edge_linear(flip)
    cases.update(nothing_cases())
    return cases
