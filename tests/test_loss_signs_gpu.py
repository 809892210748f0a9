"""Map step: the SLAM loss leaves one sign byte per pixel and the entry walk rebuilds the image gradients from it
(rtgs_slam_loss_sums_signs, RasterContext.set_loss_signs; include/rtgs_raster.h).  Kernel level: the byte plane decodes to
rtgs_slam_loss_grads' planes bit for bit.  Step level: the switch ON against OFF, with the bounds
tests/test_fused_sort_gpu.py::test_map_steps_equal_with_the_switch_on_and_off uses for two forms that differ only in
float-add order (the gradients are float-atomic sums) - and the fallbacks, which must take the float planes.  Last,
slice_publish's published statistics against the ones recorded from the commit before its loads were hoisted."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from rtg_slam_amd import _lib
from rtg_slam_amd import map_optim as mo
from rtg_slam_amd import rasterizer as rz
from rtg_slam_amd import synth
from tests import raster_util as ru

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MID = synth.CameraSpec(272, 400, 300.0, 300.0, 199.5, 135.5)      # 17 x 25 = 425 tiles: the near slice is considered
BIG = synth.CameraSpec(680, 1200, 600.0, 600.0, 599.5, 339.5)     # 43 x 75 = 3 225 tiles: 13 tiles per thread of slice_publish
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slice_publish_stats.json")


def _loss_inputs(H, W):
    """Every branch of the gradient kernel: colour differences of both signs and exactly 0, pixels without a depth owner,
    gt depth 0, depth errors below / above the threshold, negative, and exactly 0."""
    gen = torch.Generator().manual_seed(4)
    color = torch.rand(3, H, W, generator=gen)
    depth = torch.rand(1, H, W, generator=gen) * 3
    didx = torch.randint(-1, 5, (1, H, W), generator=gen, dtype=torch.int32)           # -1: a sixth of the pixels
    gt_c = torch.rand(3, H, W, generator=gen)
    gt_c[:, ::3, ::2] = color[:, ::3, ::2]                                             # sign 0 on all three channels ...
    gt_c[1, 1::3, ::4] = color[1, 1::3, ::4]                                           # ... and on one of them
    gt_d = (depth + 0.3 * torch.randn(1, H, W, generator=gen)).clamp_min(0)            # errors on both sides of 0 and of 0.1
    gt_d[0, ::5] = 0
    gt_d[0, 2::7, 1::3] = depth[0, 2::7, 1::3]                                         # error exactly 0
    rm = (torch.rand(H, W, generator=gen) < 0.6).to(torch.uint8)
    return [t.to(DEV).contiguous() for t in (color, depth, didx, gt_c, gt_d, rm)]


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("H,W", [(37, 53), (40, 52)])
def test_sign_plane_decodes_to_the_gradient_planes(H, W, masked):
    """37 x 53: the general form (odd pixel count, partial tiles); 40 x 52: the 16-byte form.  With a 60 % render mask, and
    without one at ssim_weight = 0."""
    lib = _lib.load()
    color, depth, didx, gt_c, gt_d, rm = _loss_inputs(H, W)
    if not masked:
        rm = None
    cw, dw, sw, thr = 0.8, 1.0, (0.2 if masked else 0.0), 0.1
    cfg = _lib.LossCfgC(cw, dw, sw, thr, rm.data_ptr() if rm is not None else None, 0)
    with_ssim = int(rm is None)
    nbytes = lib.rtgs_slam_loss_scratch_bytes(H, W, with_ssim)
    off = lib.rtgs_slam_loss_signs_offset(H, W, with_ssim)
    assert off % 16 == 0 and off + H * W <= nbytes
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)               # the launch clears its own header
    loss_s = torch.full((4,), float("nan"), device=DEV)
    loss_g = torch.full((4,), float("nan"), device=DEV)
    loss_ref = torch.full((4,), float("nan"), device=DEV)
    g_c, g_d = torch.empty(3, H, W, device=DEV), torch.empty(1, H, W, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(lib.rtgs_slam_loss_sums_signs(P(color), P(depth), P(didx), P(gt_c), P(gt_d), H, W, C.byref(cfg), P(scratch),
                                             P(loss_s), st), "rtgs_slam_loss_sums_signs")
    _lib.check(lib.rtgs_slam_loss_grads(P(color), P(depth), P(didx), P(gt_c), P(gt_d), H, W, C.byref(cfg), P(scratch),
                                        P(loss_g), P(g_c), P(g_d), st), "rtgs_slam_loss_grads")
    # the reference value: rtgs_slam_loss on a scratch of its own
    scratch2 = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    g_c2, g_d2 = torch.empty_like(g_c), torch.empty_like(g_d)
    _lib.check(lib.rtgs_slam_loss(P(color), P(depth), P(didx), P(gt_c), P(gt_d), H, W, C.byref(cfg), P(scratch2), P(loss_ref),
                                  P(g_c2), P(g_d2), st), "rtgs_slam_loss")
    torch.cuda.synchronize()
    sums = scratch[:32].view(torch.float32)
    # kc, kd as the kernels form them: float32, IEEE division (numpy on the host)
    f32, sh = np.float32, sums.cpu().numpy()
    kc = torch.tensor(f32(cw) * (f32(1) / (f32(3) * max(sh[3], f32(1)))), device=DEV)
    kd = torch.tensor(f32(dw) * (f32(1) / max(sh[2], f32(1))), device=DEV)
    assert kc.dtype == torch.float32 and kd.dtype == torch.float32 and sh[2] > 0 and sh[3] > 0
    signs = scratch[off:off + H * W].view(H, W).to(torch.int32)

    def decode(code, k):
        assert int(code.max()) <= 2
        zero = torch.zeros((), device=DEV)
        return torch.where(code == 1, k, torch.where(code == 2, -k, zero))
    dec_c = torch.stack([decode((signs >> (2 * c)) & 3, kc) for c in range(3)])
    dec_d = decode((signs >> 6) & 3, kd)[None]
    # every code occurs on every channel, and every gate of the depth term closes somewhere
    for c in range(4):
        assert sorted(((signs >> (2 * c)) & 3).unique().tolist()) == [0, 1, 2], c
    assert torch.equal(dec_c, g_c) and torch.equal(dec_d, g_d)
    assert torch.equal(g_c, g_c2) and torch.equal(g_d, g_d2)
    ls, lg, lr = loss_s.cpu(), loss_g.cpu(), loss_ref.cpu()
    print("loss signs, kernel level:", dict(H=H, W=W, masked=masked), ls.tolist(), lg.tolist(), lr.tolist(),
          dict(rel=[abs(float(x) - float(y)) / max(1.0, abs(float(y))) for x, y in zip(ls, lr)]))
    for x, y in zip(ls, lr):
        assert abs(float(x) - float(y)) < 2e-6 * max(1.0, abs(float(y))), (ls, lr)
    for x, y in zip(ls, lg):                                                           # same sums: rounding of the total only
        assert abs(float(x) - float(y)) < 2e-6 * max(1.0, abs(float(y))), (ls, lg)


def _render_mask(cam):
    return (torch.rand(cam.H, cam.W, generator=torch.Generator().manual_seed(9)) < 0.6).to(torch.uint8).to(DEV)


_SCENE = {}


def _scene():
    if "g" not in _SCENE:
        _SCENE["g"] = ru.make_scene(150_000, MID, seed=6)[0]
    return _SCENE["g"]


def _steps(signs, masked=True, walk=0, n_frozen=0, steps=4, lr=1e-4):
    """Four one-call map steps on the MID scene -> losses, parameters, the path counters' and the speculation's deltas."""
    g, cam = _scene(), MID
    ctx = rz.current_context()
    ctx.set_loss_signs(signs)
    ctx.set_bwd_walk(walk)
    try:
        packed = mo.pack_from_activated({k: v.to(DEV) for k, v in g.items()})
        opt = mo.ShardedMapOptimizer(packed, lr_col=mo.default_lr_columns() * lr, n_frozen=n_frozen)
        gen = torch.Generator().manual_seed(3)
        gt_c = torch.rand(3, cam.H, cam.W, generator=gen).to(DEV)
        gt_d = (1.0 + torch.rand(1, cam.H, cam.W, generator=gen)).to(DEV)
        _, s = ru.make_scene(8, cam, seed=1)
        rs = ru.hip_settings(s, DEV)
        rm = _render_mask(cam) if masked else None
        p0, s0 = ctx.loss_signs_stats(), ctx.speculation_stats()
        opt.begin_local_optimization()
        losses = [float(opt.step_slam(rs, gt_c, gt_d, None, render_mask=rm)) for _ in range(steps)]
        p1, s1 = ctx.loss_signs_stats(), ctx.speculation_stats()
        return (losses, opt.params.detach().cpu(), {k: p1[k] - p0[k] for k in p1}, {k: s1[k] - s0[k] for k in s1})
    finally:
        ctx.set_loss_signs(True)
        ctx.set_bwd_walk(0)


_OFF = {}


def _off(masked=True, walk=0, n_frozen=0):
    """The switch-off run of a configuration, computed once."""
    key = (masked, walk, n_frozen)
    if key not in _OFF:
        _OFF[key] = _steps(False, masked, walk, n_frozen)
    return _OFF[key]


def _assert_steps_equal(on, off):
    for x, y in zip(on[0], off[0]):
        assert abs(x - y) <= 1e-5 * max(1.0, abs(x)), (on[0], off[0])
    assert ru.frac_bad(on[1], off[1], 2e-6) < 1e-3


def test_map_steps_equal_with_the_switch_on_and_off():
    on, off = _steps(True), _off()
    print("loss signs, map steps:", on[0], off[0], on[2], off[2], on[3], dict(frac_bad=ru.frac_bad(on[1], off[1], 2e-6)))
    # (the first step of a process has no history to guess from; the rest speculate, and hold)
    assert on[3]["speculative"] >= 1 and off[3]["speculative"] >= 1 and on[3]["failed"] == 0 and off[3]["failed"] == 0, (on[3], off[3])
    # every step - the speculative ones among them - read signs; none did with the switch off
    assert on[2] == dict(signs=4, floats=0) and off[2] == dict(signs=0, floats=4), (on[2], off[2])
    _assert_steps_equal(on, off)


def test_ssim_live_takes_the_float_planes():
    on, off = _steps(True, masked=False), _off(masked=False)
    assert on[2] == dict(signs=0, floats=4) and off[2] == dict(signs=0, floats=4), (on[2], off[2])
    _assert_steps_equal(on, off)


def test_forced_strip_walk_takes_the_float_planes():
    on, off = _steps(True, walk=1), _off(walk=1)
    assert on[2] == dict(signs=0, floats=4) and off[2] == dict(signs=0, floats=4), (on[2], off[2])
    _assert_steps_equal(on, off)


def test_fully_frozen_map_still_returns_the_loss():
    """An empty trainable range: rendered, the loss evaluated, nothing differentiated - the value comes from the sums launch."""
    n = _scene()["xyz"].shape[0]
    on, off = _steps(True, n_frozen=n, steps=2), _steps(False, n_frozen=n, steps=2)
    print("loss signs, frozen map:", on[0], off[0], on[2], off[2])
    assert on[2]["signs"] == 2 and off[2]["signs"] == 0, (on[2], off[2])
    assert all(x == x and x > 0 for x in on[0])
    for x, y in zip(on[0], off[0]):
        assert abs(x - y) <= 1e-5 * max(1.0, abs(x)), (on[0], off[0])
    assert torch.equal(on[1], off[1])                                                  # nothing was stepped


def slice_stats(which):
    """The published near-slice statistics of one forward: `mid` = the 272 x 400 scene of the step tests in automatic slice
    mode, `big` = 150 000 Gaussians at 1200 x 680 with the slice forced (3 225 tiles: 13 per thread of slice_publish)."""
    ctx = rz.current_context()
    cam = MID if which == "mid" else BIG
    g, s = ru.make_scene(150_000, cam, seed=6)
    try:
        if which == "big":
            ctx.set_near_slice(1, 384)
        ru.hip_run(s, g)
        st = ctx.last_slice_stats()
    finally:
        ctx.set_near_slice(2, 384)
    return {k: int(st[k]) for k in ("used", "tiles_finished", "tiles_left_to_pass2", "instances")}


@pytest.mark.parametrize("which", ["mid", "big"])
def test_slice_publish_statistics_match_the_recorded_ones(which):
    want = json.load(open(GOLDEN))[which]
    got = slice_stats(which)
    print("slice_publish:", which, got)
    assert got == want
    assert got["used"] == 1 and got["instances"] > 0 and got["tiles_finished"] + got["tiles_left_to_pass2"] > 0
