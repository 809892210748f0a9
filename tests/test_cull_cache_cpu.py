"""The map epoch `ShardedMapOptimizer.step_slam` hands the one-call step (rtgs_map_step_args.map_epoch; the rasterizer
context keeps its per-row cull results from one step to the next only while the epoch stays the same): on CPU tensors,
through the bookkeeping alone (`_next_map_epoch` is what step_slam calls, `_epoch_state` what it records).

* two step_slam calls with nothing in between pass the same epoch, which is never 0;
* every public mutator that writes rows - append_rows, remove_rows, freeze_rows, step, and the switch to and from a global
  optimisation (other rows are rendered) - changes the epoch the next step_slam would pass (append_rows_masked and
  history_merge bump `version` and the row count like the others, but run device kernels only: no CPU path to call here;
  tests/test_cull_cache_gpu.py appends, removes and freezes on the device);
* begin_local_optimization leaves the rows alone and the epoch with them; new work arenas, a stale activation or a
  second rank change it."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from rtg_slam_amd import map_optim as mo  # noqa: E402
from rtg_slam_amd import synth  # noqa: E402
from tests import torch_doubles as td  # noqa: E402
from tests.dist_util import adam_reference  # noqa: E402

CAM = synth.CameraSpec(32, 48, 40.0, 40.0, 23.5, 15.5)


def _packed(n, seed):
    return mo.pack_from_activated(synth.random_gaussians(n, CAM, seed=seed))


def _opt(n=24, n_frozen=8):
    return mo.ShardedMapOptimizer(_packed(n, 1), adam_fn=adam_reference, activate_fn=td.activate8, n_frozen=n_frozen, capacity=64)


def _slam_step(opt):
    """The bookkeeping of step_slam's single-GPU path, in its order: the epoch, the version bump, the work arenas, the
    recorded state, the activation left current by the tail."""
    epoch = opt._next_map_epoch()
    opt.version += 1
    if opt._slam_ws is None:
        opt._slam_ws = dict(hw=(CAM.H, CAM.W))
    opt._epoch_seen = opt._epoch_state()
    opt._act_valid = True
    return epoch


def _loss(gd):
    return gd["xyz"].pow(2).sum() + gd["scales"].pow(2).sum()


def test_back_to_back_steps_share_one_epoch_and_it_is_never_zero():
    opt = _opt()
    first = _slam_step(opt)
    assert first != 0
    assert [_slam_step(opt) for _ in range(5)] == [first] * 5
    opt.begin_local_optimization()                       # snapshot + Adam reset: no row is written
    assert _slam_step(opt) == first


def _append(opt):
    opt.append_rows(_packed(3, 2))


def _remove(opt):
    m = torch.zeros(opt.N, dtype=torch.bool)
    m[opt.n_frozen + 1] = True
    opt.remove_rows(m, start=opt.n_frozen)


def _freeze(opt):
    m = torch.zeros(opt.N, dtype=torch.bool)
    m[opt.n_frozen + 2] = True
    opt.freeze_rows(m)


def _autograd_step(opt):
    opt.step(_loss)


def _global_on(opt):
    opt.begin_global_optimization()


def _global_off(opt):
    opt.begin_global_optimization()
    _slam_step(opt)
    opt.end_global_optimization()


def _new_arenas(opt):
    opt._slam_ws = dict(hw=(2 * CAM.H, 2 * CAM.W))       # what step_slam does when the image size changes


def _stale_activation(opt):
    opt._act_valid = False                               # raw8 moved outside the step's tail: the next step re-activates every row


def _second_rank(opt):
    opt.world = 2


@pytest.mark.parametrize("mutate", [_append, _remove, _freeze, _autograd_step, _global_on, _global_off,
                                    _new_arenas, _stale_activation, _second_rank], ids=lambda f: f.__name__.strip("_"))
def test_whatever_writes_rows_changes_the_epoch(mutate):
    opt = _opt()
    _slam_step(opt)
    e = _slam_step(opt)
    mutate(opt)
    e2 = opt._next_map_epoch()                           # what the next step_slam would pass
    assert e2 != e and e2 != 0
    opt.world = 1
    opt._act_valid = True
    opt.version += 1
    opt._epoch_seen = opt._epoch_state()
    assert _slam_step(opt) == e2                         # ... and it settles again
