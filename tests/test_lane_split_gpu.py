"""-m gpu: the lane-split launches of the fused step (csrc/oc_step_device.h: LaneParts,
env_obs_lanes; k_multi_step<..., LN = 2>) against the one-lane-per-env launch and against
``oracle.OracleBatch.multi_step``, bit for bit, every step.

With two lanes per env a workgroup covers 32 envs, the two parts of an env store different
observation rows through one store instruction (the part's distance in rows is added to the lane's
byte offset), and the state and shaping waves work in part 0 alone.  What that can get wrong: a row
stored by the wrong part, by nobody, or twice with different values; a tail lane of some part that
stores although its env does not exist; counters added once per part.  So: batch sizes around the
workgroup size (32 envs; 16 as well: four lanes per env were built and measured, lost at every batch
size and were taken out) and their tails, the straight-line comm cases and the
loop, the three observation dtypes, two levels (three subtask rows, an odd number; nine, and the
39-offset table), the observation tensor filled with a pattern before EVERY step (a row nobody
stored shows) and placed in front of a guard region (a row stored too far shows), T = 7 so that
every env times out and auto-resets five times in 40 steps, the six metrics counters, and one run as
a captured graph.  One oracle run per (level, C) at the largest batch serves every case: envs are
independent, so a smaller batch is its first n envs.
"""
import functools

import numpy as np
import pytest
import torch

from hip_util import SENTINEL, bits
from hip_util import with_margin as _with_margin

pytestmark = pytest.mark.gpu

LEVELS = ["open-divider_tomato", "full-divider_salad"]
SIZES = [1, 15, 16, 17, 31, 32, 33, 65, 100]
NMAX, STEPS, T, RADIUS = 100, 40, 7, 2
FILL = 0x6B                               # the byte every observation row holds before a step
DTYPES = {"int32": torch.int32, "int8": torch.int8, "float32": torch.float32}
COUNTERS = ("env_steps", "episodes", "successes", "reward_sum", "completed_subtasks_sum", "errors")


@functools.lru_cache(maxsize=None)
def _level(level):
    from gym_comm_amd import compiler
    return compiler.compile_level(level, 2, T)


@functools.lru_cache(maxsize=None)
def _reference(level, C):
    """Actions [STEPS][4][NMAX] and the oracle's (obs, timestep, reward, done, comm) of every step;
    computed once per (level, C), never modified."""
    from oracle import oracle
    oracle.build()
    rng = np.random.default_rng(77 + 10 * C + len(level))
    mv = rng.integers(0, 4, (STEPS, 2, NMAX)).astype(np.int32)
    cm = rng.integers(0, C, (STEPS, 2, NMAX)).astype(np.int32)
    acts = np.ascontiguousarray(np.stack([mv[:, 0], cm[:, 0], mv[:, 1], cm[:, 1]], axis=1).astype(np.int32))
    ora = oracle.OracleBatch(_level(level).blob, NMAX)
    comm = np.zeros((2, NMAX), np.int32)
    steps = []
    for k in range(STEPS):
        o, t, r, d = ora.multi_step(acts[k], comm, RADIUS, 0, C, auto_reset=True)
        steps.append((o.copy(), t.copy(), r.copy(), d.copy(), comm.copy()))
    for a in (acts,) + tuple(x for s in steps for x in s):
        a.setflags(write=False)
    return acts, steps


def _env(monkeypatch, level, n, C, dtype, lanes):
    from gym_comm_amd.batched import BatchedOvercooked
    monkeypatch.setenv("OC_LAUNCH", "lanes=%d" % lanes)
    env = BatchedOvercooked(_level(level), num_envs=n, device="cuda:0", num_communication=C,
                            fow_radius=RADIUS, auto_reset=True, obs_dtype=DTYPES[dtype])
    assert env.kernel_flavour == "spec"
    assert env.launch_waves_per_64 == 4 and env.launch_lanes() == lanes
    env.obs, margin = _with_margin(env.obs)          # (before the first step: it fixes the pointers it launches with)
    return env, margin


def _run(monkeypatch, level, n, C, dtype, lanes):
    """40 eager steps; every step compared with the oracle.  Returns what each step left in the
    output tensors (raw bytes of the observation, so a stale fill byte would show) and the counters."""
    acts, ref = _reference(level, C)
    env, margin = _env(monkeypatch, level, n, C, dtype, lanes)
    acts_d = torch.from_numpy(acts[:, :, :n].copy()).to("cuda:0")
    out = []
    for k in range(STEPS):
        env.obs.view(torch.uint8).fill_(FILL)
        o, t, r, d = env.multi_step(acts_d[k])
        oo, to, ro, do, co = (x[..., :n] for x in ref[k])
        ctx = "%s n=%d C=%d %s lanes=%d step %d" % (level, n, C, dtype, lanes, k)
        got = o.cpu().numpy()
        assert got.shape == oo.shape, ctx
        assert np.array_equal(got.astype(np.int64), oo.astype(np.int64)), ctx
        assert np.array_equal(bits(t.cpu().numpy()), bits(to)), ctx
        assert np.array_equal(bits(r.cpu().numpy()), bits(ro)), ctx
        assert np.array_equal(d.cpu().numpy(), do), ctx
        assert np.array_equal(env.comm.cpu().numpy(), co), ctx
        out.append((got.view(np.uint8).copy(), bits(t.cpu().numpy()), bits(r.cpu().numpy()), d.cpu().numpy(),
                    env.comm.cpu().numpy(), env.reward.cpu().numpy(), env.state.cpu().numpy()))
    assert bool((margin == SENTINEL).all().item()), "bytes past the last observation row were written"
    m = env.read_metrics()
    assert m["env_steps"] == n * STEPS
    assert m["episodes"] == sum(int(s[3][:n].sum()) for s in ref) >= 5 * n     # every env timed out five times
    return out, m


def _compare_forms(monkeypatch, level, n, C, dtype):
    base, m1 = _run(monkeypatch, level, n, C, dtype, 1)
    for lanes in (2,):
        got, m = _run(monkeypatch, level, n, C, dtype, lanes)
        for k, (a, b) in enumerate(zip(base, got)):
            for x, y in zip(a, b):
                assert np.array_equal(x, y), "lanes=%d differs from lanes=1 at step %d" % (lanes, k)
        assert {c: m[c] for c in COUNTERS} == {c: m1[c] for c in COUNTERS}, lanes


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("level", LEVELS)
def test_batch_sizes_around_the_workgroup(monkeypatch, level, n):
    _compare_forms(monkeypatch, level, n, 2, "int32")


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("C", [1, 2, 3, 5])
@pytest.mark.parametrize("level", LEVELS)
def test_comm_channels_and_observation_dtypes(monkeypatch, level, C, dtype):
    _compare_forms(monkeypatch, level, NMAX, C, dtype)


@pytest.mark.parametrize("lanes", [2])
def test_captured_eight_step_graph(monkeypatch, lanes):
    """The same launches as ONE captured graph of eight steps, replayed five times: 40 steps over a
    fixed window of eight action sets (the oracle steps the same window)."""
    from oracle import oracle
    level, n, C, K = "open-divider_tomato", NMAX, 2, 8
    acts, _ = _reference(level, C)
    window = acts[:K].copy()
    env, margin = _env(monkeypatch, level, n, C, "int32", lanes)
    acts_d = torch.from_numpy(window).to("cuda:0")
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        env.multi_step(acts_d[0])                     # (code objects load outside the capture)
        stream.synchronize()
        env.reset()
        env.comm.zero_()
        env.metrics.zero_()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            for k in range(K):
                env.multi_step(acts_d[k])
        ora = oracle.OracleBatch(_level(level).blob, n)
        comm = np.zeros((2, n), np.int32)
        dones = 0
        for replay in range(STEPS // K):
            env.obs.view(torch.uint8).fill_(FILL)
            graph.replay()
            stream.synchronize()
            for k in range(K):
                oo, to, ro, do = ora.multi_step(window[k], comm, RADIUS, 0, C, auto_reset=True)
                dones += int(do.sum())
            ctx = "lanes=%d after replay %d" % (lanes, replay)
            assert np.array_equal(env.obs.cpu().numpy(), oo), ctx
            assert np.array_equal(bits(env.timestep.cpu().numpy()), bits(to)), ctx
            assert np.array_equal(bits(env.shaped_reward.cpu().numpy()), bits(ro)), ctx
            assert np.array_equal(env.done.cpu().numpy(), do), ctx
            assert np.array_equal(env.comm.cpu().numpy(), comm), ctx
    assert bool((margin == SENTINEL).all().item())
    m = env.read_metrics()
    assert m["env_steps"] == n * STEPS and m["episodes"] == dones >= 5 * n and m["errors"] == 0


def test_host_reports_the_lane_choice(monkeypatch):
    """oc_multi_step_lanes: what OC_LAUNCH forces, and the library's own choice -- more than one lane
    per env only while the launch's waves find idle SIMDs, one at 131 072 envs; never for the general
    variant, and the duty split it reports beside it stays four."""
    from gym_comm_amd import specialize
    flavour, L = specialize.load_for(_level("open-divider_tomato").blob, True)
    assert flavour == "spec"
    for lanes in (1, 2):
        monkeypatch.setenv("OC_LAUNCH", "lanes=%d" % lanes)
        assert L.oc_multi_step_lanes(4096, 0, 0) == lanes and L.oc_multi_step_lanes(131072, 4, 0) == lanes
        assert L.oc_multi_step_waves(4096, 0, 0) == 4
        assert L.oc_multi_step_lanes(4096, 0, 1) == 1            # options / general variant: one lane per env
        assert L.oc_multi_step_lanes(4096, 1, 0) == 1            # an unsplit launch as well
    monkeypatch.delenv("OC_LAUNCH")
    assert L.oc_multi_step_lanes(4096, 0, 0) == 2 and L.oc_multi_step_lanes(8192, 0, 0) == 2
    assert L.oc_multi_step_lanes(8193, 0, 0) == 1
    assert L.oc_multi_step_lanes(131072, 0, 0) == 1
    assert L.oc_multi_step_waves(4096, 0, 0) == 4
    from gym_comm_amd import _lib
    assert _lib.load().oc_multi_step_lanes(4096, 0, 0) == 1      # the generic library has no such kernel

