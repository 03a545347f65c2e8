"""-m gpu: the part of a step that every arm of the step kernels executes -- env_step's proposal,
collisions, interact() and done / reward, and the auto-reset selects of multi_step_body
(csrc/oc_step_device.h) -- against ``oracle.OracleBatch``, bit for bit, every step.

Those blocks keep every per-lane predicate as a 0 / -1 word formed and consumed by single vector
instructions (bit-field extract, subtract-and-shift, bit-field insert).  What such a form can
get wrong is a predicate that only holds on part of its operand range: the sign-of-a-difference
compares are valid for operands in [0, 2^31) alone, a one-bit "held by agent a" for two agents
alone, the branch-free `timeout` for T != 0 alone.  So this file steps

  * the fused step at batch sizes around the wave and the lane-split workgroup, on two levels, in
    the three launch forms a batch can get (one lane per env, two lanes per env, one wave), with
    T = 7 (every env times out and auto-resets repeatedly) and T = 0 (no time limit: the other
    side of `timeout`; the timestep is t / 0.0: nan at t = 0, observed before the first step,
    inf after every step);
  * with action words outside the table: move codes 4, 5, -1, 2^31 - 1 and -2^31 mixed into a
    random stream of 0..3, comm indices >= C and negative ones.  Kernel and oracle flag these
    (OC_ERR_ACTION) and execute a defined result; results, flags and the `errors` counter must be
    equal, i.e. every caller-supplied value still takes the compare form;
  * the base step on a three-agent level (the shared-cell quirk of check_collisions, the
    holder compare that is no single bit for A > 2) in both launch forms, same action mix
    (there code 4 is the valid "stay");
  * a level that repeats a content type and a level with arglist.play on: other paths through the
    same selects;
  * one captured graph of eight headline-form steps, replayed five times, the observation tensor
    pre-filled and followed by a guard region.

Every input generated here was first run through the oracle alone on the CPU: it accepts all of
them -- no assertion, flags instead of faults on every out-of-table code of the list above -- so
none had to be left out.  Envs are independent: one oracle run per (level, T) at the largest
batch serves every smaller batch as its first n envs.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, compile_for, load_golden
from hip_util import SENTINEL, assert_snapshots_equal, bits
from hip_util import with_margin as _with_margin

pytestmark = pytest.mark.gpu

LEVELS = ["open-divider_tomato", "full-divider_salad"]
SIZES = [1, 31, 32, 33, 65, 100]
FORMS = ["lanes=1", "lanes=2", "split=1"]
NMAX, STEPS, C, RADIUS = 100, 60, 2, 2
FILL = 0x6B
MOVE_CODES = [0, 1, 2, 3, 4, 5, -1, 2 ** 31 - 1, -2 ** 31]
COMM_BAD = [C, C + 5, 2 ** 31 - 1, -1, -2, -2 ** 31]


def mixed_moves(rng, shape, valid_below, p_bad=0.06):
    """A random stream of valid codes 0 .. valid_below - 1 with codes of MOVE_CODES mixed in."""
    mv = rng.integers(0, valid_below, shape).astype(np.int64)
    bad = rng.random(shape) < p_bad
    return np.where(bad, rng.choice(MOVE_CODES, size=shape), mv).astype(np.int32)


def mixed_comm(rng, shape, p_bad=0.04):
    cm = rng.integers(0, C, shape).astype(np.int64)
    bad = rng.random(shape) < p_bad
    return np.where(bad, rng.choice(COMM_BAD, size=shape), cm).astype(np.int32)


def fused_actions(seed, steps=STEPS, n=NMAX):
    """[steps][4][n]: ego move, ego comm, alt move, alt comm."""
    rng = np.random.default_rng(seed)
    mv = mixed_moves(rng, (steps, 2, n), 4)
    cm = mixed_comm(rng, (steps, 2, n))
    return np.ascontiguousarray(np.stack([mv[:, 0], cm[:, 0], mv[:, 1], cm[:, 1]], axis=1))


def base_actions(seed, A, steps=STEPS, n=NMAX):
    """[steps][A][n] NAV codes: 0..4 valid (4 = stay), the rest of MOVE_CODES flagged."""
    return np.ascontiguousarray(mixed_moves(np.random.default_rng(seed), (steps, A, n), 5))


@functools.lru_cache(maxsize=None)
def _level(level, A, T):
    from gym_comm_amd import compiler
    return compiler.compile_level(level, A, T)


def oracle_fused(lv, acts, n):
    """The oracle's (obs, timestep, reward, done, comm, raised a flag) of every step."""
    from oracle import oracle
    oracle.build()
    ora = oracle.OracleBatch(lv.blob, n)
    comm = np.zeros((2, n), np.int32)
    steps = []
    for k in range(acts.shape[0]):
        o, t, r, d = ora.multi_step(acts[k], comm, RADIUS, 0, C, auto_reset=True)
        raised = ora.last_step()["raised"]
        steps.append((o.copy(), t.copy(), r.copy(), d.copy(), comm.copy(), raised.copy()))
    for s in steps:
        for x in s:
            x.setflags(write=False)
    return steps


@functools.lru_cache(maxsize=None)
def _reference(level, T):
    acts = fused_actions(900 + 13 * T + len(level))
    acts.setflags(write=False)
    return acts, oracle_fused(_level(level, 2, T), acts, NMAX)


def _fused_env(monkeypatch, lv, n, form, **kw):
    from gym_comm_amd.batched import BatchedOvercooked
    monkeypatch.setenv("OC_LAUNCH", form)
    env = BatchedOvercooked(lv, num_envs=n, device="cuda:0", num_communication=C, fow_radius=RADIUS,
                            auto_reset=True, **kw)
    assert env.kernel_flavour == "spec"
    env.obs, margin = _with_margin(env.obs)
    return env, margin


def _check_fused(env, margin, acts, ref, n, ctx0):
    acts_d = torch.from_numpy(np.ascontiguousarray(acts[:, :, :n])).to("cuda:0")
    raised = 0
    for k in range(acts.shape[0]):
        env.obs.view(torch.uint8).fill_(FILL)
        o, t, r, d = env.multi_step(acts_d[k])
        oo, to, ro, do, co, ra = (x[..., :n] for x in ref[k])
        ctx = "%s step %d" % (ctx0, k)
        assert np.array_equal(o.cpu().numpy(), oo), ctx
        assert np.array_equal(bits(t.cpu().numpy()), bits(to)), ctx
        assert np.array_equal(bits(r.cpu().numpy()), bits(ro)), ctx
        assert np.array_equal(d.cpu().numpy(), do), ctx
        assert np.array_equal(env.comm.cpu().numpy(), co), ctx
        raised += int((ra != 0).sum())
    assert bool((margin == SENTINEL).all().item()), "bytes past the last observation row were written"
    m = env.read_metrics()
    assert m["env_steps"] == n * acts.shape[0], ctx0
    assert m["episodes"] == sum(int(s[3][:n].sum()) for s in ref), ctx0
    assert m["errors"] == raised, ctx0
    return m


@pytest.mark.parametrize("T", [7, 0])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("level", LEVELS)
def test_fused_step_with_action_words_outside_the_table(monkeypatch, level, n, form, T):
    acts, ref = _reference(level, T)
    env, margin = _fused_env(monkeypatch, _level(level, 2, T), n, form)
    want = dict(kv.split("=") for kv in form.split(","))
    if "lanes" in want:
        assert env.launch_waves_per_64 == 4 and env.launch_lanes() == int(want["lanes"])
    else:
        assert env.launch_waves_per_64 == 1
    if T == 0:
        # t / 0.0 at t = 0, seen before the first step: nan.  (Not compared bit for bit with the
        # oracle: the reference itself raises ZeroDivisionError here, the oracle's C division gives
        # the x86 default NaN, sign bit set, and the kernels have always written the positive quiet
        # NaN.  Those bits are what is pinned.)
        from oracle import oracle
        _, ts0 = env.observe()
        _, et = oracle.OracleBatch(_level(level, 2, T).blob, 1).obs(0, 0, RADIUS, False, False, C, np.zeros(2, np.int32))
        assert np.isnan(et) and (bits(ts0.cpu().numpy()) == 0x7FF8000000000000).all()
    m = _check_fused(env, margin, acts, ref, n, "%s n=%d %s T=%d" % (level, n, form, T))
    dones = sum(int(s[3][:n].sum()) for s in ref)
    if T == 7:
        assert dones >= (STEPS // T) * n               # every env timed out again and again
    else:
        assert dones == 0 and all(np.isinf(s[1][:n]).all() for s in ref)   # no time limit: t / 0.0
    # the mix did reach the flags (a property of the generated stream, equal for kernel and oracle)
    assert n < 31 or m["errors"] > 0


def oracle_base(lv, acts, n):
    """Base-step reference.  The oracle steps WITHOUT auto-reset and is reset by hand where an
    episode ended, so that the flags an env-step raised are seen before the reset clears them: per
    step (reward, done, shaping, snapshot after the reset), and the number of env-steps that raised
    a flag (the flag word differs from before: what the `errors` counter counts)."""
    from oracle import oracle
    oracle.build()
    ora = oracle.OracleBatch(lv.blob, n)
    steps, raised = [], []
    prev = np.zeros(n, np.int32)
    for k in range(acts.shape[0]):
        r, d, sh = ora.step(acts[k], auto_reset=False)
        raised.append(ora.snapshot_all()["error"] != prev)
        if d.any():
            ora.reset(d)
        snap = ora.snapshot_all()
        prev = snap["error"].copy()
        steps.append((r.copy(), d.copy(), sh.copy(), snap))
    return steps, raised


def _check_base(monkeypatch, lv, acts, ref, n, form):
    from gym_comm_amd.batched import BatchedOvercooked
    steps, raised = ref
    monkeypatch.setenv("OC_LAUNCH", form)
    env = BatchedOvercooked(lv, num_envs=n, device="cuda:0", auto_reset=True)
    assert env.kernel_flavour == "spec"
    acts_d = torch.from_numpy(np.ascontiguousarray(acts[:, :, :n])).to("cuda:0")
    was = np.zeros(n, bool)
    for k in range(acts.shape[0]):
        r, d, sh = env.step(acts_d[k])
        ro, do, sho, snap = steps[k]
        ctx = "%s n=%d %s step %d" % (lv.name, n, form, k)
        hs = env.snapshot()
        err = snap["error"][:n]
        assert np.array_equal(hs["error"], err), ctx
        # (an env whose reference store is corrupt -- OC_ERR_ALIAS, bit 1 -- is left out until its
        # episode has ended, as in test_hip_parity; OC_ERR_ACTION has a defined result and stays in)
        clean = ((err & 2) == 0) & ~was
        was = (err & 2) != 0
        assert np.array_equal(r.cpu().numpy()[clean], ro[:n][clean]), ctx
        assert np.array_equal(d.cpu().numpy()[clean], do[:n][clean]), ctx
        assert np.array_equal(bits(sh.cpu().numpy())[:, clean], bits(sho)[:, :n][:, clean]), ctx
        assert_snapshots_equal(hs, {key: v[:n] for key, v in snap.items()}, ctx, where=clean)
    m = env.read_metrics()
    assert m["env_steps"] == n * acts.shape[0]
    assert m["episodes"] == sum(int(s[1][:n].sum()) for s in steps)
    assert m["errors"] == sum(int(x[:n].sum()) for x in raised)
    return m


N3 = 130


@functools.lru_cache(maxsize=None)
def _reference_base3():
    """partial-divider_tl, three agents, T = 9, the largest batch."""
    lv = _level("partial-divider_tl", 3, 9)
    acts = base_actions(4103, 3, n=N3)
    acts.setflags(write=False)
    return lv, acts, oracle_base(lv, acts, N3)


@pytest.mark.parametrize("form", ["step_split=1", "step_split=2"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, N3])
def test_base_step_three_agents(monkeypatch, n, form):
    lv, acts, ref = _reference_base3()
    m = _check_base(monkeypatch, lv, acts, ref, n, form)
    assert n < 63 or m["errors"] > 0


def _fixture_level(name):
    _, st = load_golden(os.path.join(GOLDEN, name))
    return compile_for(st)


# one level that repeats a content type (DUP kernels), one recorded with arglist.play on (PM): both
# from tests/spec_levels.py, so their libraries are pre-built
@pytest.mark.parametrize("name,flag", [("cwrap_dup_two_lettuces_salad_c3.npz", "has_dup"),
                                       ("pwrap_play_salad_c3.npz", "play")])
def test_dup_level_and_play(monkeypatch, name, flag):
    lv = _fixture_level(name)
    assert getattr(lv, flag) and lv.num_agents == 2
    n = NMAX
    # the fused step ...
    acts = fused_actions(77 + len(name))
    ref = oracle_fused(lv, acts, n)
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    from gym_comm_amd.batched import BatchedOvercooked
    env = BatchedOvercooked(lv, num_envs=n, device="cuda:0", num_communication=C, fow_radius=RADIUS, auto_reset=True)
    assert env.kernel_flavour == "spec"
    env.obs, margin = _with_margin(env.obs)
    _check_fused(env, margin, acts, ref, n, name)
    # ... and the base step
    bacts = base_actions(78 + len(name), 2)
    _check_base(monkeypatch, lv, bacts, oracle_base(lv, bacts, n), n, "step_split=2")


def test_captured_eight_step_graph(monkeypatch):
    """The headline form (open-divider_tomato, two lanes per env) as ONE captured graph of eight
    steps, replayed five times over a fixed window of eight action sets."""
    from oracle import oracle
    oracle.build()
    level, n, K, T = "open-divider_tomato", NMAX, 8, 7
    lv = _level(level, 2, T)
    window = fused_actions(31, steps=K)
    env, margin = _fused_env(monkeypatch, lv, n, "lanes=2")
    assert env.launch_waves_per_64 == 4 and env.launch_lanes() == 2
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
        ora = oracle.OracleBatch(lv.blob, n)
        comm = np.zeros((2, n), np.int32)
        dones = raised = 0
        for replay in range(5):
            env.obs.view(torch.uint8).fill_(FILL)
            graph.replay()
            stream.synchronize()
            for k in range(K):
                oo, to, ro, do = ora.multi_step(window[k], comm, RADIUS, 0, C, auto_reset=True)
                dones += int(do.sum())
                raised += int((ora.last_step()["raised"] != 0).sum())
            ctx = "after replay %d" % replay
            assert np.array_equal(env.obs.cpu().numpy(), oo), ctx
            assert np.array_equal(bits(env.timestep.cpu().numpy()), bits(to)), ctx
            assert np.array_equal(bits(env.shaped_reward.cpu().numpy()), bits(ro)), ctx
            assert np.array_equal(env.done.cpu().numpy(), do), ctx
            assert np.array_equal(env.comm.cpu().numpy(), comm), ctx
            assert_snapshots_equal(env.snapshot(), ora.snapshot_all(), ctx)
    assert bool((margin == SENTINEL).all().item())
    m = env.read_metrics()
    assert m["env_steps"] == n * 5 * K and m["episodes"] == dones >= 5 * n and m["errors"] == raised > 0
