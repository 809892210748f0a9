"""loop_closure_rotate_sh end to end on the drifted turn of tests/test_loop_closure_gpu.py: with the key the closure turns the map's
higher SH bands by the definition of rtgs_map_deform_sh and changes nothing else; absent or False it never calls the kernel.

The turn is mapped ONCE; every closure starts from the same restored state (trajectory, keyframes, kept normals, the map's rows
with seeded higher bands), so the closures can be compared value for value."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import sh_rotation as shr
from tests import map_deform_reference as mdr
from tests import map_deform_sh_reference as msr
from tests.test_loop_closure_gpu import CAM, DEV, drifted_poses, frames, loop_args
from tests.test_map_deform_gpu import bits

pytestmark = pytest.mark.gpu
BLOCKS = ("xyz", "shs", "raw8")
_run = {}


def mapped_turn():
    """-> (mapper, tracker, snapshot) of the drifted turn, the higher SH bands of the live rows filled with seeded normal values
    of sigma 0.05; mapped once."""
    if not _run:
        from rtg_slam_amd import slam
        fr = frames()
        drifted = drifted_poses([f[2] for f in fr])
        torch.manual_seed(1)
        stream = ((d, c, drifted[k]) for k, (d, c, _) in enumerate(fr))
        mapper, tracker, rep = slam.run_sequence(CAM, stream, loop_args(), DEV, capacity=200_000)
        assert "loop_closure" not in rep
        opt = mapper.opt
        opt.flush()
        N = int(opt.N)
        bands = torch.randn(N, 45, generator=torch.Generator().manual_seed(5)) * 0.05
        opt.state["shs"]["p"][:N, 3:] = bands.to(DEV)
        snap = {"poses": [np.array(p, dtype=np.float64) for p in tracker.pose_es], "N": N,
                "rows": {k: opt.state[k]["p"][:N].clone() for k in BLOCKS},
                "normals": [km["normal_map_w"].clone() if "normal_map_w" in km else None for km in mapper.keymap_list]}
        _run.update(mapper=mapper, tracker=tracker, snap=snap)
    return _run["mapper"], _run["tracker"], _run["snap"]


def restore(mapper, tracker, snap):
    tracker.pose_es[:] = [p.copy() for p in snap["poses"]]
    mapper.update_poses(tracker.pose_es)
    for km, n in zip(mapper.keymap_list, snap["normals"]):
        if n is not None:
            km["normal_map_w"] = n.clone()
    opt = mapper.opt
    opt.flush()
    assert int(opt.N) == snap["N"]
    for k in BLOCKS:
        opt.state[k]["p"][:snap["N"]].copy_(snap["rows"][k])
    opt._act_valid = False


def close(**over):
    """One closure from the restored state -> (report, rows after as numpy, poses after, the recorded deform_rows arguments)."""
    mapper, tracker, snap = mapped_turn()
    restore(mapper, tracker, snap)
    opt, seen = mapper.opt, []
    real = opt.deform_rows

    def recording(table, tick=None, sh_table=None):
        used = opt.aux["add_tick"] if tick is None else tick
        seen.append({"table": table.cpu().numpy().copy(), "tick": used.reshape(-1)[:snap["N"]].cpu().numpy().copy(),
                     "sh_table": None if sh_table is None else sh_table.cpu().numpy().copy()})
        return real(table, tick=tick, sh_table=sh_table) if sh_table is not None else real(table, tick=tick)
    opt.deform_rows = recording
    try:
        rep = lc.LoopCloser(loop_args(**over)).close(mapper, tracker)
    finally:
        del opt.deform_rows
    torch.cuda.synchronize()
    rows = {k: opt.state[k]["p"][:snap["N"]].cpu().numpy() for k in BLOCKS}
    return rep, rows, np.stack(tracker.pose_es), seen


def timeless(x):
    """A report without its clock readings."""
    if isinstance(x, dict):
        return {k: timeless(v) for k, v in x.items() if k not in ("seconds", "device_s")}
    if isinstance(x, (list, tuple)):
        return [timeless(v) for v in x]
    return x


def count_calls(monkeypatch):
    from rtg_slam_amd import _lib
    lib = _lib.load()
    calls = [0]
    real = lib.rtgs_map_deform_sh

    def counted(*a):
        calls[0] += 1
        return real(*a)
    monkeypatch.setattr(lib, "rtgs_map_deform_sh", counted)
    return calls


def test_on_turns_the_sh_block_by_the_definition_and_changes_nothing_else(monkeypatch):
    calls = count_calls(monkeypatch)
    snap = mapped_turn()[2]
    before = {k: v.cpu().numpy() for k, v in snap["rows"].items()}
    rep_off, rows_off, poses_off, seen_off = close()
    assert calls[0] == 0
    rep, rows, poses, seen = close(loop_closure_rotate_sh=True)
    assert calls[0] == 1 and len(seen) == 1 and len(seen_off) == 1
    assert rep["changed"] and rep["edges"] >= 1 and rep["sh_rotated"] is True and rep["seconds"]["sh_table"] >= 0
    table, tick, sh_table = seen[0]["table"], seen[0]["tick"], seen[0]["sh_table"]
    assert sh_table.dtype == np.float32 and sh_table.shape == (table.shape[0], 84) and seen_off[0]["sh_table"] is None
    # the SH block is the definition applied to the block before, with the tick and the table the closure passed
    want = msr.deform_sh(before["shs"].reshape(-1, 16, 3), tick, sh_table).reshape(-1, 48)
    assert np.array_equal(bits(rows["shs"]), bits(want))
    turned = sh_table[np.clip(tick.astype(np.int64), 0, sh_table.shape[0] - 1), 83] != 0
    assert turned.any() and not np.array_equal(bits(rows["shs"][turned, 3:]), bits(before["shs"][turned, 3:]))
    assert np.array_equal(bits(rows["shs"][:, :3]), bits(before["shs"][:, :3]))                     # the DC term
    # flag 0 exactly where the map's own table holds the identity row; the blocks are those of the table's rotation
    identity = (table == mdr.IDENTITY_ROW).all(axis=1)
    assert identity[0] and not identity.all()
    assert np.array_equal(sh_table[:, 83] == 0, identity) and set(np.unique(sh_table[:, 83])) <= {0.0, 1.0}
    for f in np.linspace(0, table.shape[0] - 1, 8).astype(int):
        R = table[f].astype(np.float64).reshape(4, 4)[:3, :3]
        blocks = np.concatenate([m.reshape(-1) for m in shr.sh_rotation_blocks(R)])
        assert np.abs(sh_table[f, :83] - blocks).max() < 1e-6, f
    # everything else is the closure without the key
    assert np.array_equal(poses, poses_off)
    assert np.array_equal(bits(rows["xyz"]), bits(rows_off["xyz"])) and np.array_equal(bits(rows["raw8"]), bits(rows_off["raw8"]))
    assert np.array_equal(seen[0]["table"], seen_off[0]["table"]) and np.array_equal(seen[0]["tick"], seen_off[0]["tick"])
    mine = timeless(rep)
    assert mine.pop("sh_rotated") is True
    assert mine == timeless(rep_off)
    assert set(rep["seconds"]) - set(rep_off["seconds"]) == {"sh_table"}


def test_off_leaves_the_sh_block_alone(monkeypatch):
    calls = count_calls(monkeypatch)
    snap = mapped_turn()[2]
    before = snap["rows"]["shs"].cpu().numpy()
    for over in ({}, {"loop_closure_rotate_sh": False}):
        rep, rows, _, seen = close(**over)
        assert rep["changed"] and rep["edges"] >= 1                              # the map did move ...
        assert not np.array_equal(bits(rows["xyz"]), bits(snap["rows"]["xyz"].cpu().numpy()))
        assert np.array_equal(bits(rows["shs"]), bits(before))                   # ... its SH block did not
        assert "sh_rotated" not in rep and "sh_table" not in rep["seconds"] and seen[0]["sh_table"] is None
        assert "rotate_sh" not in rep["options"]
    assert calls[0] == 0


def test_a_value_that_is_no_bool_is_refused():
    for bad in ("yes", 1, 0, None, "true"):
        with pytest.raises(ValueError):
            lc.LoopCloser(loop_args(loop_closure_rotate_sh=bad))
    assert lc.LoopCloser(loop_args(loop_closure_rotate_sh=True)).rotate_sh is True
    assert lc.LoopCloser(loop_args()).rotate_sh is False and "loop_closure_rotate_sh" not in lc.DEFAULTS
