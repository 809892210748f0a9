"""Where a Gauss-Newton launch of the tracker spends its time: per-wave stamps (rtgs_icp_set_stamps, include/rtgs_debug.h) of
the 15 residual launches of ONE 3-level x 5-iteration track, on tools/prof_icp.py's frames.
    python tools/icp_stamps.py [replica|tum] [last-arriver]
Prints per level (mean over its 5 launches): launch span (first wave in -> last wave out), the mean wave's lifetime and its
phases in us.  Head-solve chain (default): head sum (the previous launch's rows, float64) | head solve (+ the barrier
behind it) - both per workgroup, mean over all waves - | source loads | gathers | projection, gates, sums | the row's store.  The solve of the LAST iteration runs in icp_p2p, which carries no
stamps.  `last-arriver` (RTGS_ICP_FLAG_LAST_ARRIVER): source loads | gathers | compute | publish + ticket, and the last
arriver's partial reads + float64 sum and solve.  Shader cycles are converted at the clock the stamps themselves show
(cycles / wall time)."""
import math
import os
import sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtg_slam_amd import _lib, synth, icp as hicp

LAUNCHES, WGS = 16, 256           # RTGS_ICP_STAMP_LAUNCHES, RTGS_ICP_STAMP_WGS
cam = synth.REPLICA if (len(sys.argv) < 2 or sys.argv[1] == "replica") else synth.TUM_FR1
OLD = "last-arriver" in sys.argv[2:]
lib = _lib.load()
dev = torch.device("cuda", 0)
poses = synth.trajectory(2, seed=9)
base = synth.look_at_pose(seed=3, max_angle_deg=5, max_trans=0.3)
d0 = synth.box_room_depth(cam, base @ poses[0]).to(dev)
d1 = synth.box_room_depth(cam, base @ poses[1]).to(dev)
K = torch.tensor([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], dtype=torch.float32, device=dev)
vp0, np0 = hicp.build_pyramids(d0, K, 3)
vp1, np1 = hicp.build_pyramids(d1, K, 3)
cos_thr = math.cos(math.radians(20.0))
track = lambda: hicp.icp_track(vp1, np1, vp0, np0, K, [0.25, 0.5, 1.0], [5, 5, 5], 0.1, cos_thr, 1e-4, last_arriver=OLD)
for _ in range(20):
    track()
torch.cuda.synchronize()
runs = []
for rep in range(5):
    st = torch.zeros(LAUNCHES * WGS * 4 * 8, dtype=torch.int64, device=dev)
    lib.rtgs_icp_set_stamps(st.data_ptr())
    out = track()
    torch.cuda.synchronize()
    lib.rtgs_icp_set_stamps(None)
    runs.append(st.cpu().numpy().reshape(LAUNCHES, WGS, 4, 8).astype(np.int64))
    track()                                              # an unstamped track between the stamped ones
torch.cuda.synchronize()

print(f"{cam.H}x{cam.W}: per-wave stamps of the residual launches, mean of {len(runs)} tracks; us")
print(("last-arriver chain\n" if OLD else "head-solve chain\n") +
      "level  px       WGs  span   wave_life | src_loads gathers  compute  publish | " + ("last: sum   solve" if OLD else "head: sum   solve") + " | gap_to_next")
rows = []
for s in runs:
    per = []
    for k in range(15):
        w = s[k]
        live = w[:, :, 0] > 0
        t_in, t_out = w[:, :, 0][live], w[:, :, 1][live]
        span = (t_out.max() - t_in.min()) * 0.01
        life = (t_out - t_in) * 0.01
        if OLD:
            plain = live & (w[:, :, 6] == 0)                         # waves without the last arriver's work
            cyc_total = (w[:, :, 2] + w[:, :, 3] + w[:, :, 4] + w[:, :, 5])[plain]
        else:                                                        # every wave has a head; its cycles are stamped too
            plain = live
            cyc_total = w[:, :, 2:8].sum(-1)[plain]
        ghz = (cyc_total.sum() / max(((w[:, :, 1] - w[:, :, 0])[plain] * 0.01).sum(), 1e-9)) * 1e-3   # cycles per us -> GHz
        mhz = ghz * 1e3
        ph = [float(w[:, :, c][live].mean()) / mhz for c in (2, 3, 4, 5)]
        if OLD:
            lastw = w[:, 0, 6] > 0
            fin = [float(w[lastw, 0, 6].mean()) / mhz, float(w[lastw, 0, 7].mean()) / mhz] if lastw.any() else [0.0, 0.0]
        else:                                                        # launch 0 of a track has no head to run: zeros
            fin = [float(w[:, :, 6][live].mean()) / mhz, float(w[:, :, 7][live].mean()) / mhz]
        nxt = s[k + 1] if k + 1 < 15 else None
        gap = ((nxt[:, :, 0][nxt[:, :, 0] > 0].min() - t_out.max()) * 0.01) if nxt is not None else float("nan")
        per.append([int(live.any(1).sum()), span, float(life.mean())] + ph + fin + [gap, ghz])
    rows.append(per)
r = np.array(rows).mean(0)
for l in range(3):
    m = r[5 * l:5 * l + 5].mean(0)
    n = vp1[l].shape[0] * vp1[l].shape[1]
    print(f"  {l}  {n:7d}  {int(m[0]):4d}  {m[1]:5.1f}  {m[2]:6.1f}    | {m[3]:7.2f}  {m[4]:7.2f}  {m[5]:7.2f}  {m[6]:7.2f} | {m[7]:6.2f} {m[8]:6.2f} | {m[9]:5.2f}")
tot = r[:, 1].sum()
print(f"sum of the 15 launch spans {tot:.1f} us; gaps between launches {np.nansum(r[:, 9]):.1f} us; shader clock from the "
      f"stamps {r[:, 10].mean():.2f} GHz; stats {out[16:].tolist()}")
