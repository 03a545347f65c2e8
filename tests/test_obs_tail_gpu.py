"""-m gpu: the observation rows of the fused step (csrc/oc_step_device.h: RowsPreT, env_obs, the
observation duties of multi_step_body) against ``oracle.OracleBatch.multi_step``, bit for bit.

A split launch's observation waves hold the byte offset of every row they store in a scalar
register formed before the workgroup's barrier, store the comm one-hots straight-line for up to four
channels (a loop beyond), and take the fresh episode of an auto-reset by a select.  What that can
get wrong is a row landing in the wrong place -- or outside the tensor -- for some channel count,
element size or launch policy.  So: n = 101 (one full wave and a ragged one), 40 steps, every
C in 1..5 (four unrolled forms and the loop), the three observation dtypes, the library's own launch
choice and both forced ones (four waves per 64 envs; one), the canonical subtask order and a
permuted one -- with the observation, comm and timestep tensors placed inside larger allocations
whose bytes past the last row must come back untouched.
T = 7: every env times out and auto-resets five times in 40 steps.  T = 40 with the
level's solve script as a prefix: subtasks do get completed, so the completed_subtasks rows -- the only
rows the subtask order moves -- are not all zero.
"""
import functools

import numpy as np
import pytest
import torch

from hip_util import SENTINEL, bits, scripted_then_random
from hip_util import with_margin as _with_margin

pytestmark = pytest.mark.gpu

LEVEL, N, STEPS, RADIUS = "open-divider_tomato", 101, 40, 2
ORDERS = {"canonical": None, "permuted": [2, 0, 1]}
DTYPES = {"int32": torch.int32, "int8": torch.int8, "float32": torch.float32}
LAUNCHES = {"auto": None, "split4": "split=4", "split1": "split=1"}


@functools.lru_cache(maxsize=None)
def _level(T, order):
    from gym_comm_amd import compiler
    return compiler.compile_level(LEVEL, 2, T, subtask_order=ORDERS[order])


@functools.lru_cache(maxsize=None)
def _reference(T, C, order):
    """The actions of one (T, C, order) case and what the oracle returns for every step of them;
    computed once, shared by the dtype x launch cases, never modified."""
    from oracle import oracle
    oracle.build()
    lv = _level(T, order)
    rng = np.random.default_rng(1000 * T + 10 * C + len(order))
    if T > STEPS - 1:
        mv = scripted_then_random(rng, LEVEL, STEPS, 2, N, nact=4)
    else:
        mv = rng.integers(0, 4, (STEPS, 2, N)).astype(np.int32)
    cm = rng.integers(0, C, (STEPS, 2, N)).astype(np.int32)
    acts = np.ascontiguousarray(np.stack([mv[:, 0], cm[:, 0], mv[:, 1], cm[:, 1]], axis=1).astype(np.int32))
    ora = oracle.OracleBatch(lv.blob, N)
    comm = np.zeros((2, N), np.int32)
    steps = []
    for k in range(STEPS):
        o, t, r, d = ora.multi_step(acts[k], comm, RADIUS, 0, C, auto_reset=True)
        steps.append((o.copy(), t.copy(), r.copy(), d.copy(), comm.copy()))
    for a in (acts,) + tuple(x for s in steps for x in s):
        a.setflags(write=False)
    return acts, steps


def _run(monkeypatch, T, C, order, dtype, launch):
    from gym_comm_amd.batched import BatchedOvercooked
    if LAUNCHES[launch] is None:
        monkeypatch.delenv("OC_LAUNCH", raising=False)
    else:
        monkeypatch.setenv("OC_LAUNCH", LAUNCHES[launch])
    acts, steps = _reference(T, C, order)
    env = BatchedOvercooked(_level(T, order), num_envs=N, device="cuda:0", num_communication=C,
                            fow_radius=RADIUS, auto_reset=True, obs_dtype=DTYPES[dtype])
    assert env.launch_waves_per_64 == {"auto": 4, "split4": 4, "split1": 1}[launch]
    margins = {}
    for name in ("obs", "comm", "timestep"):     # (before the first step: it fixes the pointers it launches with)
        t, margins[name] = _with_margin(getattr(env, name))
        setattr(env, name, t)
    acts_d = torch.from_numpy(acts).to("cuda:0")
    c_lo, c_hi = env._layout["completed_subtasks"]
    seen_completed = False
    for k in range(STEPS):
        o, t, r, d = env.multi_step(acts_d[k])
        oo, to, ro, do, co = steps[k]
        ctx = "step %d" % k
        got = o.cpu().numpy()
        assert got.shape == oo.shape, ctx
        assert np.array_equal(got.astype(np.int64), oo.astype(np.int64)), ctx
        assert np.array_equal(bits(t.cpu().numpy()), bits(to)), ctx
        assert np.array_equal(bits(r.cpu().numpy()), bits(ro)), ctx
        assert np.array_equal(d.cpu().numpy(), do), ctx
        assert np.array_equal(env.comm.cpu().numpy(), co), ctx
        seen_completed |= bool(oo[:, c_lo:c_hi].any())
    for name, m in margins.items():
        assert bool((m == SENTINEL).all().item()), "bytes past the last row of %s were written" % name
    return seen_completed, steps


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5])
def test_rows_with_frequent_auto_resets(monkeypatch, C, order, dtype, launch):
    _, steps = _run(monkeypatch, 7, C, order, dtype, launch)
    resets = sum(int(s[3].sum()) for s in steps)
    assert resets >= 5 * N                     # every env timed out, and started over, five times


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("C", [2, 3, 5])
def test_completed_subtask_rows_in_the_callers_order(monkeypatch, C, order, launch):
    seen, _ = _run(monkeypatch, 40, C, order, "int32", launch)
    assert seen                                # the scripted prefix completed subtasks: the rows are not all zero
