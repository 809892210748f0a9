"""The kernels of csrc/mesh_texture.hip against tests/mesh_texture_reference.py, bit for bit: levels, offsets and origins, the
texel-to-face map, the texture coordinates, the float accumulators after every view, the image, the flags and both counts."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import meshing, synth
from tests import mesh_texture_reference as tr, visibility_reference as vr

pytestmark = pytest.mark.gpu
F32 = np.float32


def _quarter_replica():
    c = synth.REPLICA
    return synth.CameraSpec(c.H // 4, c.W // 4, c.fx / 4, c.fy / 4, (c.cx + 0.5) / 4 - 0.5, (c.cy + 0.5) / 4 - 0.5)


CAM = _quarter_replica()                           # 170 x 300
K = (CAM.fx, CAM.fy, CAM.cx, CAM.cy)
BLIND = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 100.0], [0, 0, 0, 1]])       # far outside, looking away: sees nothing


def _images(n, seed):
    """n colour images of white noise: neighbouring pixels differ, so a wrong footprint or weight shows in the bits."""
    rng = np.random.default_rng(seed)
    return [rng.random((3, CAM.H, CAM.W), dtype=F32) for _ in range(n)]


def _room_poses():
    return [p.numpy() for p in synth.trajectory(3, seed=1, max_rot_deg=60.0, max_trans=0.1)]


def _compare(v, f, colors, poses, images, texel, tolerance, transform=None, **kw):
    """Reference and kernels on the same inputs; every intermediate compared.  -> (reference dict, stats of texture_mesh)."""
    T = np.eye(4) if transform is None else np.asarray(transform, dtype=np.float64)
    ref = tr.texture_mesh(v, f, colors, K, CAM.H, CAM.W, [(img, T @ p) for img, p in zip(images, poses)], texel, tolerance, **kw)
    dev = torch.device("cuda", 0)
    tv, tf_ = torch.from_numpy(np.ascontiguousarray(v, dtype=F32)).to(dev), torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).to(dev)
    tc = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors, dtype=F32)).to(dev)
    timg = [torch.from_numpy(img).to(dev) for img in images]
    baker = meshing.TextureBaker(tv, tf_, CAM, texel=texel, tolerance=tolerance, transform=transform, **kw)
    lay = ref["layout"]
    assert baker.size == (lay["Wt"], lay["Ht"]) and baker.T == lay["T"]
    assert np.array_equal(baker.levels.cpu().numpy(), ref["levels"])
    assert np.array_equal(baker.capped.cpu().numpy(), ref["capped"])
    assert np.array_equal(baker.offset.cpu().numpy(), lay["offset"])
    assert np.array_equal(baker.origin.cpu().numpy(), lay["origin"])
    assert np.array_equal(baker.texel_face.cpu().numpy(), ref["texel_face"])
    assert np.array_equal(baker.uv.cpu().numpy().view(np.uint32), ref["uv"].view(np.uint32))
    for i, (img, p) in enumerate(zip(timg, poses)):
        baker.add(img, p)
        acc = baker.acc.cpu().numpy()
        assert np.array_equal(acc.view(np.uint32), ref["acc"][i].view(np.uint32)), f"accumulators after view {i}"
    image, flags = baker.finish(tc)
    assert np.array_equal(image.cpu().numpy(), ref["image"]) and np.array_equal(flags.cpu().numpy(), ref["flags"])
    image2, uv2, stats = meshing.texture_mesh(tv, tf_, tc, CAM, zip(timg, poses), texel=texel, tolerance=tolerance, transform=transform, **kw)
    assert image2.dtype == torch.uint8 and tuple(image2.shape) == (lay["Ht"], lay["Wt"], 3) and torch.equal(image2, image)
    assert uv2.dtype == torch.float32 and tuple(uv2.shape) == (len(f), 3, 2) and torch.equal(uv2, baker.uv)
    assert stats["size"] == [lay["Wt"], lay["Ht"]] and stats["views"] == len(poses)
    assert stats["texels_assigned"] == ref["texels_assigned"] == lay["T"] and stats["texels_seen"] == ref["texels_seen"]
    assert stats["fill"] == lay["T"] / (lay["Wt"] * lay["Ht"]) and stats["faces_capped"] == int(ref["capped"].sum())
    assert stats["seen_share"] == ref["texels_seen"] / ref["texels_assigned"]
    max_level = kw.get("max_level", 6)
    assert stats["levels"] == np.bincount(ref["levels"], minlength=max_level + 1)[1:max_level + 1].tolist()
    assert stats["bake_s"] > 0 and stats["render_s"] > 0 and stats["layout_s"] > 0
    return ref, stats


@pytest.mark.parametrize("cell,texel", [(1.0, 0.05), (1.0, 0.02), (0.5, 0.05), (0.5, 0.02)])
def test_room(cell, texel):
    v, f = vr.box_grid(vr.ROOM_HALF, cell=cell)
    assert len(f) == (252 if cell == 1.0 else 1008)
    rng = np.random.default_rng(11)
    colors = rng.random((len(v), 3), dtype=F32)
    ref, stats = _compare(v, f, colors, _room_poses(), _images(3, 7), texel, 0.02)
    assert 0 < ref["texels_seen"] < ref["texels_assigned"]                      # three views leave walls unseen: the fallback runs
    if cell == 1.0 and texel == 0.02:
        assert stats["faces_capped"] == 252                                     # the diagonal, 1.41 m, is over 63 texels of 2 cm
    if cell == 0.5 and texel == 0.02:
        assert stats["size"] == [2048, 2048] and stats["faces_capped"] == 0


def _soup():
    """Faces of every level 1..6 and capped ones at a texel of 1 cm, in shuffled order, each with vertices of its own, at random
    places and orientations (both windings) 1.5 to 3 m in front of the camera; T = 32 128 gives a 256 x 128 atlas.  The last
    face crosses the near plane (one corner behind the camera): the renderer drops it whole."""
    rng = np.random.default_rng(2)
    counts = {1: 96, 2: 64, 3: 32, 4: 16, 5: 4, 6: 2, 7: 2}                      # 7: capped
    edge = {1: 0.005, 2: 0.025, 3: 0.06, 4: 0.12, 5: 0.25, 6: 0.5, 7: 1.0}      # level l: ((2^(l-1) - 1), (2^l - 1)] texels
    want = [min(l, 6) for l, n in counts.items() for _ in range(n)]
    lengths = [edge[l] for l, n in counts.items() for _ in range(n)]
    perm = rng.permutation(len(want))
    verts, levels = [], []
    for k in perm:
        e = lengths[k]
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        centre = np.array([rng.uniform(-1.2, 1.2), rng.uniform(-0.7, 0.7), rng.uniform(1.5, 3.0)])
        local = np.array([[0, 0, 0], [e, 0, 0], [0.4 * e, 0.6 * e, 0]])
        verts.append(centre + local @ q.T)
        levels.append(want[k])
    verts.append(np.array([[-0.3, -0.2, 2.0], [0.4, -0.2, 2.2], [0.0, 0.1, -1.0]]))      # 3 m long: capped, level 6
    levels.append(6)
    v = np.concatenate(verts).astype(F32)
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return v, f, np.asarray(levels, dtype=np.int32)


def test_every_level_and_a_rectangular_atlas():
    v, f, levels = _soup()
    rng = np.random.default_rng(4)
    colors = rng.random((len(v), 3), dtype=F32)
    poses = [np.eye(4), BLIND, synth.se3_exp(torch.tensor([0.0, 0.3, 0.1, -0.5, 0.1, -0.4])).numpy()]
    ref, stats = _compare(v, f, colors, poses, _images(3, 9), 0.01, 0.02)
    assert np.array_equal(ref["levels"], levels) and stats["faces_capped"] == 3 and all(n > 0 for n in stats["levels"])
    assert len(f) == 217 and ref["layout"]["T"] == 32128 and stats["size"] == [256, 128], "the atlas is rectangular"
    assert np.array_equal(ref["acc"][1], ref["acc"][0]), "the blind view adds nothing"
    assert ref["texels_seen"] > 0


def test_degenerate_and_nan_faces():
    v, f = vr.box_grid((1.0, 1.0, 2.0), cell=0.5)
    extra = np.array([[0.2, 0.1, 1.0], [0.2, 0.1, 1.0], [0.2, 0.1, 1.0],           # no extent
                      [0.0, 0.0, 1.0], [0.3, 0.0, 1.0], [0.6, 0.0, 1.0],           # no area: the cosine is NaN
                      [0.1, 0.1, 1.2], [np.nan, 0.2, 1.2], [0.3, 0.4, 1.2],        # a NaN corner
                      [0.1, -0.3, 1.2], [np.inf, 0.2, 1.2], [0.3, 0.4, 1.2]], dtype=F32)
    n = len(v)
    v = np.concatenate([v, extra])
    f = np.concatenate([f, n + np.arange(12, dtype=np.int32).reshape(4, 3)])
    rng = np.random.default_rng(8)
    colors = rng.random((len(v), 3), dtype=F32)
    ref, stats = _compare(v, f, colors, [np.eye(4), _room_poses()[2]], _images(2, 3), 0.03, 0.02)
    assert ref["levels"][-4:].tolist() == [1, 5, 1, 1] and ref["capped"][-4:].sum() == 0
    tf = ref["texel_face"]
    for face in range(len(f) - 4, len(f)):
        assert (ref["flags"][tf == face] == tr.ASSIGNED).all()                  # none of them is ever seen


def test_transform_without_colours_and_a_lower_max_level():
    v, f = vr.box_grid(vr.ROOM_HALF, cell=1.0)
    transform = synth.se3_exp(torch.tensor([0.4, -0.2, 0.3, 0.5, -0.3, 0.2])).numpy()
    v_moved = (v.astype(np.float64) @ transform[:3, :3].T + transform[:3, 3]).astype(F32)    # the room in another frame
    ref, stats = _compare(v_moved, f, None, _room_poses(), _images(3, 5), 0.05, 0.02, transform=transform, max_level=4, min_cos=0.35)
    assert stats["faces_capped"] == 252 and stats["levels"] == [0, 0, 0, 252] and 0 < ref["texels_seen"] < ref["texels_assigned"]
    assert (ref["image"][ref["flags"] == tr.ASSIGNED] == 128).all()


def test_one_face_no_face():
    dev = torch.device("cuda", 0)
    v = np.array([[-0.5, -0.4, 2], [0.6, -0.3, 2], [-0.4, 0.5, 2]], dtype=F32)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    ref, stats = _compare(v, f, np.eye(3, dtype=F32), [np.eye(4)], _images(1, 1), 0.05, 0.01)
    assert stats["size"] == [32, 32] and stats["fill"] == 1.0 and 0 < stats["texels_seen"]
    image, uv, stats = meshing.texture_mesh(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev), None, CAM,
                                            [(torch.from_numpy(_images(1, 1)[0]).to(dev), np.eye(4))], texel=0.05, tolerance=0.01)
    assert tuple(image.shape) == (1, 1, 3) and image.dtype == torch.uint8 and int(image.sum()) == 0 and image.is_cuda
    assert tuple(uv.shape) == (0, 3, 2) and stats["size"] == [1, 1] and stats["texels_assigned"] == 0 and stats["texels_seen"] == 0
    assert stats["fill"] == 0 and stats["seen_share"] == 0 and stats["views"] == 1 and stats["faces_capped"] == 0


def test_two_runs_give_equal_bytes():
    dev = torch.device("cuda", 0)
    v, f, _ = _soup()
    tv, tf_ = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    views = [(torch.from_numpy(img).to(dev), p) for img, p in zip(_images(2, 9), [np.eye(4), _room_poses()[1]])]
    runs = [meshing.texture_mesh(tv, tf_, None, CAM, views, texel=0.01, tolerance=0.02) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert {k: runs[0][2][k] for k in ("size", "texels_assigned", "texels_seen", "levels")} == \
           {k: runs[1][2][k] for k in ("size", "texels_assigned", "texels_seen", "levels")}


def test_refusals():
    dev = torch.device("cuda", 0)
    v, f = vr.box_grid(vr.ROOM_HALF, cell=1.0)
    tv, tf_ = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    img = torch.from_numpy(_images(1, 1)[0])
    with pytest.raises(RuntimeError, match="HIP device"):
        meshing.texture_mesh(torch.from_numpy(v), tf_, None, CAM, [], texel=0.05, tolerance=0.02)
    with pytest.raises(RuntimeError, match="HIP device"):
        meshing.texture_mesh(tv, tf_, None, CAM, [(img, np.eye(4))], texel=0.05, tolerance=0.02)
    with pytest.raises(RuntimeError, match="HIP device"):
        meshing.texture_mesh(tv, tf_, torch.zeros(len(v), 3), CAM, [], texel=0.05, tolerance=0.02)
    for bad in ({"texel": 0.0}, {"texel": float("nan")}, {"texel": float("inf")}, {"tolerance": 0.0}, {"tolerance": float("nan")},
                {"max_level": 0}, {"max_level": 7}):
        with pytest.raises(ValueError):
            meshing.texture_mesh(tv, tf_, None, CAM, [], **{"texel": 0.05, "tolerance": 0.02, **bad})
    with pytest.raises(ValueError, match="must be"):
        meshing.texture_mesh(tv, tf_, None, CAM, [(img[:, :50].to(dev), np.eye(4))], texel=0.05, tolerance=0.02)
    # 70 000 faces of level 6 hold 2.9e8 texels, over 16384^2 = 2.7e8: refused before anything of that size is allocated
    big_v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=torch.float32, device=dev)
    big_f = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev).repeat(70000, 1)
    with pytest.raises(ValueError, match=r"T = 286720000 texels.*smallest texel that fits is 0\.0\d+ m"):
        meshing.texture_mesh(big_v, big_f, None, CAM, [], texel=0.001, tolerance=0.02)
