"""The sparse brick TSDF volume on the MI355X (rtg_slam_amd.meshing.SparseTsdfVolume; include/rtgs_slam.h "meshing",
rtgs_tsdf_sparse_*) against its numpy definition (tests/tsdf_sparse_reference.py) bit for bit - slot order, planes, mesh - and
against the dense kernels, on a virtual grid no dense volume can hold, and at its refusals."""
import functools

import numpy as np
import pytest
import torch

from rtg_slam_amd import _lib, meshing, synth
from tests import tsdf_reference as tr
from tests import tsdf_sparse_reference as ts

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DIMS = (96, 64, 112)


@functools.lru_cache(maxsize=None)
def _inputs():
    cam, frames = ts.three_frames()
    return cam, tuple(frames), tuple((d.to(DEV), c.to(DEV), p) for d, c, p in frames)


def _volume(dims, lo=ts.THREE_LO, voxel=ts.THREE_VOXEL, cls=meshing.SparseTsdfVolume, **kw):
    hi = [l + n * voxel for l, n in zip(lo, dims)]
    vol = cls(lo, hi, voxel, device=DEV, **kw)
    assert vol.dims == tuple(dims), vol.dims
    return vol


def _fuse(vol, seq):
    cam, _, on_device = _inputs()
    for k in seq:
        d, c, p = on_device[k]
        vol.integrate(d, c, cam, p)
    return vol


@functools.lru_cache(maxsize=None)
def _reference(dims, seq, max_weight=64.0):
    cam, frames, _ = _inputs()
    vol, stats = ts.fuse_sparse(cam, [(frames[k][0].numpy(), frames[k][1].numpy(), frames[k][2]) for k in seq], ts.THREE_LO, dims,
                                ts.THREE_VOXEL, np.float32(4 * ts.THREE_VOXEL), max_weight)
    print("reference:", dims, seq, stats)
    return vol


def _assert_planes_equal(got, want):
    for name, g, w in zip(("tsdf", "weight", "rgb"), got, want):
        g, w = g.cpu(), torch.from_numpy(np.ascontiguousarray(w))
        bad = int((g.view(torch.int32) != w.view(torch.int32)).sum())
        print(name, "differing values:", bad, "of", w.numel())
        assert g.shape == w.shape and bad == 0, (name, bad)


def _assert_meshes_equal(got, want, allow_empty=False):
    gv, gf, gc, gk = (t.cpu().numpy() for t in got)
    wv, wf, wc, wk = want
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and gc.dtype == np.float32 and gk.dtype == np.int64
    print("V", len(gv), len(wv), "F", len(gf), len(wf))
    assert len(gv) == len(wv) and len(gf) == len(wf) and (allow_empty or len(gf) > 0)
    assert np.array_equal(gk, wk)
    assert np.array_equal(gf, wf)                                 # the order itself: (cell, tetrahedron, triangle), vertices by key
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32))
    assert np.array_equal(gc.view(np.uint32), wc.view(np.uint32))


@pytest.mark.parametrize("dims", [DIMS, (61, 45, 83), (93, 59, 109)])
def test_kernels_match_the_numpy_reference(dims):
    """Three frames: slot order, planes and mesh (min_weight 1 and 2) bit for bit.  (61, 45, 83) is grazed by two of the frames
    only; (93, 59, 109) cuts the last brick of every axis where the walls are."""
    ref = _reference(dims, (0, 1, 2))
    vol = _fuse(_volume(dims), (0, 1, 2))
    assert vol.frames == 3 and vol.n_bricks == ref.n_bricks > 0
    assert vol.brick_dims == ts.brick_dims(dims)
    assert vol.brick_coords.dtype == torch.int32 and torch.equal(vol.brick_coords.cpu(), torch.from_numpy(ref.brick_coords))
    if dims == DIMS:
        assert vol.n_bricks == 309
    assert vol.capacity >= vol.n_bricks and vol.bytes == 4 * int(np.prod(vol.brick_dims)) + vol.capacity * 10240
    _assert_planes_equal(vol.to_dense(), ref.to_dense())
    for min_weight in (1, 2):
        # no cell of the grazed grid has all 8 corners seen twice: both meshes are empty there
        _assert_meshes_equal(vol.extract_mesh(min_weight, return_keys=True), ref.extract(min_weight), allow_empty=min_weight == 2)
    v, f, c = vol.extract_mesh()
    assert v.shape[1] == 3 and f.dtype == torch.int32 and c.shape == v.shape
    with pytest.raises(ValueError, match="min_weight > 0"):
        vol.extract_mesh(0)


def test_max_weight_saturates():
    seq = (0,) * 7
    ref = _reference(DIMS, seq, 4.0)
    assert ref.weight.max() == 4
    vol = _fuse(_volume(DIMS, max_weight=4), seq)
    assert torch.equal(vol.brick_coords.cpu(), torch.from_numpy(ref.brick_coords)) and vol.n_bricks == 210
    _assert_planes_equal(vol.to_dense(), ref.to_dense())
    _assert_meshes_equal(vol.extract_mesh(return_keys=True), ref.extract())


def _allocated_voxels(vol):
    b = vol.brick_coords.long()
    nbx, nby, nbz = vol.brick_dims
    a = torch.zeros(nbz, nby, nbx, dtype=torch.bool, device=DEV)
    a[b[:, 2], b[:, 1], b[:, 0]] = True
    for axis in range(3):
        a = a.repeat_interleave(8, dim=axis)
    nx, ny, nz = vol.dims
    return a[:nz, :ny, :nx]


@pytest.mark.parametrize("dims", [DIMS, (93, 59, 109)])
def test_one_frame_equals_the_dense_kernels(dims):
    """The one-frame theorems on the two sets of kernels: every allocated voxel equals TsdfVolume's, and the meshes are equal
    in all four arrays.  Unallocated voxels read fresh."""
    for k in (0, 1, 2):
        sparse = _fuse(_volume(dims), (k,))
        dense = _fuse(_volume(dims, cls=meshing.TsdfVolume), (k,))
        alloc = _allocated_voxels(sparse)
        t, w, c = sparse.to_dense()
        assert 0 < int(alloc.sum()) < alloc.numel()
        assert torch.equal(t[alloc].view(torch.int32), dense.tsdf[alloc].view(torch.int32))
        assert torch.equal(w[alloc], dense.weight[alloc])
        assert torch.equal(c[:, alloc].view(torch.int32), dense.rgb[:, alloc].view(torch.int32))
        assert bool((t[~alloc] == 1).all()) and bool((w[~alloc] == 0).all()) and bool((c[:, ~alloc] == 0).all())
        got, want = sparse.extract_mesh(return_keys=True), dense.extract_mesh(return_keys=True)
        assert got[1].shape[0] > 0
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a, b)


def test_box_room_through_mesh_from_map():
    """The 20-frame box-room case (2 cm, 260 x 160 x 110) through mesh_from_map with both volumes: V, F and the wall statistics
    are equal, 2 243 of 9 240 bricks are allocated, and the pool - its CAPACITY, growth slack included: at most 1.5 times the
    allocated bricks' 0.25 of the dense planes - stays under half the dense planes."""
    cam, frames, lo, hi, voxel = tr.box_room_case()
    stream = [(d.to(DEV), c.to(DEV), p) for d, c, p in frames]
    kw = dict(voxel=voxel, depth_source="sensor", bounds=(lo, hi), device=DEV)
    sv, sf, sc, sparse = meshing.mesh_from_map(None, cam, None, iter(stream), volume="sparse", **kw)
    dv, df, dc, dense = meshing.mesh_from_map(None, cam, None, iter(stream), **kw)
    print("sparse:", sparse)
    print("dense:", dense)
    assert set(sparse) - set(dense) == {"volume", "bricks", "brick_share", "pool_bytes", "dense_bytes"} and set(dense) <= set(sparse)
    assert sparse["volume"] == "sparse" and sparse["dims"] == dense["dims"] == [260, 160, 110] and sparse["frames_fused"] == 20
    assert (sparse["V"], sparse["F"]) == (dense["V"], dense["F"]) == (sv.shape[0], sf.shape[0]) and sparse["F"] > 0
    got, want = tr.wall_stats(sv.cpu().numpy()), tr.wall_stats(dv.cpu().numpy())
    print("sparse:", got, "dense:", want)
    assert got == want
    assert sparse["bricks"] == 2243 and abs(sparse["brick_share"] - 2243 / 9240) < 1e-12
    assert sparse["dense_bytes"] == 260 * 160 * 110 * 20
    print("pool / dense bytes:", sparse["pool_bytes"] / sparse["dense_bytes"])
    assert 2243 * 10240 <= sparse["pool_bytes"] < 0.5 * sparse["dense_bytes"]


HUGE_CAM = synth.CameraSpec(24, 32, 200.0, 200.0, 15.5, 11.5)
HUGE_LO, HUGE_VOXEL, HUGE_DIMS = (-2.56, -2.56, -2.06), 0.0025, (2048, 2048, 2048)
HUGE_WINDOW = ((880, 1168), (912, 1136), (1976, 2048))


def test_a_virtual_grid_no_dense_volume_can_hold():
    """2048^3 voxels of 2.5 mm (8.6e9 voxels, 172 GB of dense planes, a brick table of 2^24 entries) around a 24 x 32 frame
    that sees a 0.48 x 0.36 m patch of the far wall at 2.97-3.00 m.  The voxels' linear indices are around 8.4e9, past 2^31
    and 2^32.  The reference evaluates the window x [880, 1168), y [912, 1136), z [1976, 2048) with the true indices (and
    asserts that no in-band voxel touches the window's inner faces)."""
    pose = torch.eye(4, dtype=torch.float64)
    depth = synth.box_room_depth(HUGE_CAM, pose)
    color = synth.box_room_color(HUGE_CAM, pose, depth)
    depth = depth.reshape(HUGE_CAM.H, HUGE_CAM.W).contiguous()
    assert 2.9 < float(depth.min()) and float(depth.max()) < 3.01
    hi = [l + n * HUGE_VOXEL for l, n in zip(HUGE_LO, HUGE_DIMS)]
    with pytest.raises(ValueError, match="GiB"):
        meshing.TsdfVolume(HUGE_LO, hi, HUGE_VOXEL, device=DEV)
    vol = meshing.SparseTsdfVolume(HUGE_LO, hi, HUGE_VOXEL, device=DEV)
    assert vol.dims == HUGE_DIMS and vol.brick_dims == (256, 256, 256) and vol.dense_bytes == 20 * 2048 ** 3
    vol.integrate(depth.to(DEV), color.to(DEV), HUGE_CAM, pose.numpy())
    ref, stats = ts.fuse_sparse(HUGE_CAM, [(depth.numpy(), color.numpy(), pose.numpy())], HUGE_LO, HUGE_DIMS, HUGE_VOXEL,
                                np.float32(4 * HUGE_VOXEL), window=HUGE_WINDOW)
    print("reference:", stats, "bricks", ref.n_bricks, "pool MB", ref.n_bricks * 10240 / 1e6)
    b = vol.brick_coords.cpu()
    assert vol.n_bricks == ref.n_bricks > 1000
    for axis, (a0, a1) in enumerate(HUGE_WINDOW):
        assert int(b[:, axis].min()) * 8 >= a0 and int(b[:, axis].max()) * 8 + 8 <= a1
    assert torch.equal(b, torch.from_numpy(ref.brick_coords))
    _assert_planes_equal(vol.to_dense(HUGE_WINDOW), ref.to_dense())
    want = ref.extract()
    _assert_meshes_equal(vol.extract_mesh(return_keys=True), want)
    assert want[3].min() // 7 > 2 ** 32                              # the keys' linear indices are past 32 bits
    assert vol.bytes < 1 << 28                                       # 64 MiB of table and some 12 MB of pool, for 172 GB of grid
    with pytest.raises(ValueError, match="GiB"):
        vol.to_dense()
    with pytest.raises(ValueError, match="window"):
        vol.to_dense(((0, 8), (0, 8), (2040, 2049)))


def test_a_frame_without_valid_depth_allocates_nothing():
    cam, _, on_device = _inputs()
    vol = _volume(DIMS)
    vol.integrate(torch.zeros(cam.H, cam.W, device=DEV), on_device[0][1], cam, on_device[0][2])
    assert vol.frames == 1 and vol.n_bricks == 0 and vol.brick_coords.shape == (0, 3) and vol.pool_bytes == 0
    v, f, c, k = vol.extract_mesh(return_keys=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3) and k.shape == (0,) and f.dtype == torch.int32
    t, w, c = vol.to_dense()
    assert bool((t == 1).all()) and bool((w == 0).all()) and bool((c == 0).all())
    # and the volume still works afterwards
    _fuse(vol, (0,))
    assert vol.n_bricks == 210


def test_over_the_cap_raises_before_anything_is_written():
    table_bytes = 4 * int(np.prod(ts.brick_dims(DIMS)))
    need = table_bytes + 210 * 10240                                   # the first frame allocates 210 bricks
    vol = _volume(DIMS, max_bytes=need - 1)
    with pytest.raises(ValueError, match=r"210 bricks, 2\.05 MiB of pool and 0\.01 MiB of brick table, over the cap of 2\.06 MiB"):
        _fuse(vol, (0,))
    assert vol.n_bricks == 0 and vol.frames == 0 and vol.pool_bytes == 0
    assert bool((vol._table == -1).all())
    assert vol.extract_mesh()[1].shape[0] == 0
    exact = _fuse(_volume(DIMS, max_bytes=need), (0,))
    assert exact.n_bricks == 210 and exact.bytes == need
    with pytest.raises(ValueError, match="over the cap"):              # the second frame needs more
        _fuse(exact, (1,))
    assert exact.n_bricks == 210 and exact.frames == 1
    with pytest.raises(ValueError, match="dense copy of 96 x 64 x 112"):   # to_dense answers to the same cap
        exact.to_dense()
    free = _fuse(_volume(DIMS), (0,))                                   # the refused frame left the first one's bricks as they were
    assert torch.equal(exact.brick_coords, free.brick_coords) and torch.equal(exact._table, free._table)
    assert torch.equal(exact._pool[:210].view(torch.int32), free._pool[:210].view(torch.int32))


def test_two_runs_are_bit_equal():
    a, b = _fuse(_volume(DIMS), (0, 1, 2)), _fuse(_volume(DIMS), (0, 1, 2))
    assert a.n_bricks == b.n_bricks == 309
    assert torch.equal(a.brick_coords, b.brick_coords) and torch.equal(a._table, b._table)
    assert torch.equal(a._pool[:a.n_bricks].view(torch.int32), b._pool[:b.n_bricks].view(torch.int32))
    for x, y in zip(a.extract_mesh(return_keys=True), b.extract_mesh(return_keys=True)):
        assert torch.equal(x, y)


def test_bad_arguments_return_minus_one():
    lib = _lib.load()
    vol = _fuse(_volume(DIMS), (0,))
    p = lambda t: t.data_ptr()
    counts = torch.zeros(vol.n_bricks * 512, dtype=torch.int32, device=DEV)
    ok = lambda **kw: lib.rtgs_tsdf_sparse_count(kw.get("pool", p(vol._pool)), p(vol._coords), p(vol._table), kw.get("n", vol.n_bricks),
                                                 kw.get("nx", 96), 64, 112, kw.get("min_weight", 1.0), p(counts), None)
    assert ok() == 0
    assert ok(pool=None) == -1 and ok(n=-1) == -1 and ok(nx=0) == -1 and ok(nx=2 ** 24 + 1) == -1 and ok(min_weight=0.0) == -1
    assert lib.rtgs_tsdf_sparse_allocate(p(vol._table), p(vol._flags), p(vol._flags), 96, 64, 112, vol.n_bricks, 1, vol.n_bricks,
                                         p(vol._coords), p(vol._pool), None) == -1          # past the capacity
    w6 = (_lib.C.c_int32 * 6)(0, 8, 0, 8, 0, 113)
    t = torch.zeros(8, device=DEV)
    assert lib.rtgs_tsdf_sparse_to_dense(p(vol._pool), p(vol._table), 96, 64, 112, w6, p(t), p(t), p(t), None) == -1
    torch.cuda.synchronize()
