"""rtg_slam_amd.evaluation.exposure_aware_picture and the exposure_aware rows of eval_frame / evaluate_sequence: the render is
brought into the frame's own exposure and white balance by the kernels of csrc/white_balance.hip (source = the render, target =
the frame) and scored by the existing picture_metrics.  tests/white_balance_reference.py is the definition of the correction."""
import numpy as np
import pytest
import torch

from tests import test_map_exposure_gpu as grey_gpu
from tests import test_white_balance_cpu as cpu
from tests import white_balance_reference as wbr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
GAINS, OFFSETS = (1.25, 0.8, 1.1), (-0.06, 0.08, 0.02)
EVAL_GATES = dict(src_lo=-np.inf, src_hi=np.inf, dst_lo=4 / 255, dst_hi=251 / 255)
MIN_DEPTH, MAX_DEPTH = 0.1, 8.0
dev = grey_gpu.dev


def size():
    from rtg_slam_amd import evaluation as ev
    return max(176, ev.MS_SSIM_MIN_SIDE + 1), 200                               # MS-SSIM's smaller side must exceed MS_SSIM_MIN_SIDE


def picture(frame_of_render):
    """A render of wbr.textured at depth 2 (one pixel above 1, which only a correction clamps) and the frame made of it."""
    H, W = size()
    render = wbr.textured(H, W)
    render[0, 0, 0] = 1.2
    frame = frame_of_render(render)
    d = np.full((H, W), 2.0, F32)
    out = {"render": dev(render), "depth": dev(d[None]), "T_map": dev(np.zeros((1, H, W), F32)),
           "depth_index_map": dev(np.zeros((1, H, W), np.int32))}
    return render, frame, d, out


def noisy(r):
    """The render under GAINS / OFFSETS plus sensor noise of 0.02 and 5 % of the pixels a random colour: a finite PSNR either way."""
    rng = np.random.default_rng(3)
    f = wbr.tinted(r, GAINS, OFFSETS) + rng.normal(0, 0.02, r.shape).astype(F32)
    hit = rng.random(r.shape[1:]) < 0.05
    return np.clip(np.where(hit[None], rng.uniform(0.05, 0.95, r.shape).astype(F32), f), 0, 1).astype(F32)


def test_known_gains_are_returned_and_the_corrected_psnr_exceeds_the_plain_one():
    """On a frame that is exactly the render under a known gain and offset per channel: the gains and offsets are the known ones
    within the recovery bound of tests/test_white_balance_cpu.py, and the corrected render is the frame (up to the clamp)."""
    from rtg_slam_amd import evaluation as ev
    render, frame, d, out = picture(lambda r: wbr.tinted(r, GAINS, OFFSETS))
    res = ev.exposure_aware_picture(out, dev(frame), dev(d), MIN_DEPTH, MAX_DEPTH, True)
    plain = ev.eval_picture(out, dev(frame), dev(d), MIN_DEPTH, MAX_DEPTH, True)
    print(f"psnr {plain['psnr']:.3f} -> {res['psnr_ea']:.3f} dB, gains {[res['gain_' + c] for c in 'rgb']}, offsets "
          f"{[res['offset_' + c] for c in 'rgb']}, bound {cpu.recovery_bound():.3g}")
    assert res["code"] == 0 and res["psnr_ea"] > plain["psnr"] and res["color_l1_ea"] < plain["color_l1"]
    for c, name in enumerate("rgb"):
        assert abs(res["gain_" + name] - GAINS[c]) <= cpu.recovery_bound()
        assert abs(res["offset_" + name] - OFFSETS[c]) <= cpu.recovery_bound()


def test_figures_are_picture_metrics_of_the_definitions_corrected_render():
    from rtg_slam_amd import evaluation as ev
    render, frame, d, out = picture(noisy)
    res = ev.exposure_aware_picture(out, dev(frame), dev(d), MIN_DEPTH, MAX_DEPTH, True)
    plain = ev.eval_picture(out, dev(frame), dev(d), MIN_DEPTH, MAX_DEPTH, True)
    ab, codes, code, _ = wbr.fit(render, d, frame, d, np.zeros_like(d), **EVAL_GATES)
    corrected, _ = wbr.apply(render, ab)
    v = ev.picture_metrics(dev(corrected), dev(frame), out["depth"], dev(d), out["depth_index_map"], MIN_DEPTH, MAX_DEPTH,
                           True).cpu().tolist()
    print(f"psnr {plain['psnr']:.3f} -> {res['psnr_ea']:.3f} dB, ssim {plain['ssim']:.4f} -> {res['ssim_ea']:.4f}")
    assert np.isfinite([res["psnr_ea"], res["ssim_ea"], res["color_l1_ea"]]).all()
    assert code == wbr.OK and codes == [wbr.OK] * 4 and res["code"] == 0
    assert res["psnr_ea"] == v[ev.OUT_PSNR] and res["ssim_ea"] == v[ev.OUT_MS_SSIM] and res["color_l1_ea"] == v[ev.OUT_COLOR_L1]
    for c, name in enumerate("rgb"):
        assert res["gain_" + name] == ab[c + 1][0] and res["offset_" + name] == ab[c + 1][1]
        assert abs(res["gain_" + name] - GAINS[c]) <= cpu.grey_cpu.SCHEDULE_BOUND    # the bound at 20 % outliers; here 5 % and noise
    assert res["psnr_ea"] > plain["psnr"] and res["color_l1_ea"] < plain["color_l1"]
    assert set(res) == {"psnr_ea", "ssim_ea", "color_l1_ea", "gain_r", "gain_g", "gain_b", "offset_r", "offset_g", "offset_b", "code"}
    no_ms = ev.exposure_aware_picture(out, dev(frame), dev(d), MIN_DEPTH, MAX_DEPTH, False)
    assert no_ms["ssim_ea"] is None and no_ms["psnr_ea"] == res["psnr_ea"]
    with pytest.raises(ValueError, match="unknown exposure gate"):
        ev.exposure_aware_picture(out, dev(frame), dev(d), MIN_DEPTH, MAX_DEPTH, True, lo=0.0)


def test_a_refused_fit_returns_the_plain_figures():
    from rtg_slam_amd import evaluation as ev
    render, frame, d, out = picture(lambda r: wbr.tinted(r, GAINS, OFFSETS))
    plain = ev.eval_picture(out, dev(frame), dev(d), MIN_DEPTH, MAX_DEPTH, True)
    res = ev.exposure_aware_picture(out, dev(frame), dev(d), MIN_DEPTH, MAX_DEPTH, True, min_valid=10 ** 9)
    assert res["code"] == wbr.TOO_FEW
    assert (res["psnr_ea"], res["ssim_ea"], res["color_l1_ea"]) == (plain["psnr"], plain["ssim"], plain["color_l1"])
    assert [res["gain_" + c] for c in "rgb"] == [1.0] * 3 and [res["offset_" + c] for c in "rgb"] == [0.0] * 3
    flat = np.full_like(render, 0.5)                                            # a frame without variance is no target either
    out["render"] = dev(flat)
    res = ev.exposure_aware_picture(out, dev(frame), dev(d), MIN_DEPTH, MAX_DEPTH, True)
    plain = ev.eval_picture(out, dev(frame), dev(d), MIN_DEPTH, MAX_DEPTH, True)
    assert res["code"] == wbr.FLAT and res["psnr_ea"] == plain["psnr"]


def test_evaluate_sequence_keeps_its_keys_and_puts_the_new_rows_apart():
    from rtg_slam_amd import evaluation as ev
    mapper, _, _, _, _, _ = grey_gpu._run(grey_gpu._args(gaussian_update_iter=5), None, n=3)
    cam = grey_gpu._cam()
    gains = [torch.tensor(g, device=DEV).reshape(3, 1, 1) for g in ((1.0, 1.0, 1.0), (1.2, 0.9, 1.05), (0.85, 1.1, 0.95))]
    stream = lambda: ((d, (c * gains[k]).clamp(0, 1), c2w) for k, (d, c, c2w) in enumerate(grey_gpu._frames(3)))
    off = ev.evaluate_sequence(mapper, cam, stream())
    on = ev.evaluate_sequence(mapper, cam, stream(), exposure_aware=True)
    row_keys = {"valid_pixel_ratio", "depth_loss", "normal_loss", "psnr", "ssim", "lpips", "color_l1", "frame", "iter"}
    assert set(off) == {"rows", "mean"} and all(set(r) == row_keys for r in off["rows"])
    assert set(on) == {"rows", "mean", "exposure_rows", "exposure_mean", "exposure_seconds"}
    assert on["rows"] == off["rows"] and on["mean"] == off["mean"]
    assert [set(r) for r in on["exposure_rows"]] == [{"frame", "psnr"} | set(ev.EXPOSURE_ROW_KEYS)] * 3
    for k, r in enumerate(on["exposure_rows"]):
        print(f"frame {k}: psnr {r['psnr']:.3f} -> {r['psnr_ea']:.3f} dB, gains {r['gain_r']:.4f} {r['gain_g']:.4f} {r['gain_b']:.4f}")
        assert r["code"] == 0 and r["psnr"] == off["rows"][k]["psnr"]
        if k > 0:
            assert r["psnr_ea"] > r["psnr"]
            for c, name in enumerate("rgb"):
                g = float(gains[k][c])
                assert abs(r["gain_" + name] - g) < abs(1 - g)
    assert on["exposure_mean"]["frames_refused"] == 0 and on["exposure_mean"]["psnr_ea"] > on["exposure_mean"]["psnr"]
    assert on["exposure_seconds"] > 0
