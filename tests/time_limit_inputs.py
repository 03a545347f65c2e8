"""Inputs shared by test_time_limit_gpu.py and test_time_limit_inputs_cpu.py -- not a test module, and
nothing here touches a device on import.

The GPU tests run the step counter t and the time limit T over the whole width of their 16-bit
fields (include/oc_hip.h: t lives in bits 16..31 of state row 0, next to agent 0's cell and held
item; T <= 65535): the episode is started at a chosen t by writing those bits after reset() and the
oracle follows with ``OracleBatch.set_t``.  The CPU test checks with the oracle alone that ``set_t``
equals real stepping and that the inputs built here reach what the GPU cases are about.

  LIMITS           the time limits: field edges, the sign bit of row 0, one odd value, and 0 (no limit)
  start_values     env i's first t: a fixed list, cycled and clipped to [0, T - 1]
  fused_actions    [STEPS][4][n]: hip_util.scripted_then_random (moves 0..3) with seeded comm indices;
                   every fourth env plays SOLVE, the level's solve script without a "stay", to its end
  base_actions     [STEPS][3][n] NAV codes for the three-agent base step
  fused_reference  / base_reference: the oracle's run of an input, computed once, read-only

STEPS is 26 and not 12: open-divider_tomato cannot be delivered in 12 joint steps from reset (a
breadth-first search over all 16 joint moves per step with the oracle reaches 311 987 distinct states
at depth 12 and none of them is done; the known solve takes 23), and a batch whose t alone is injected
starts from reset.  So the window is the solve plus three steps, which changes nothing about the
time-outs the start values are chosen for.
"""
import functools

import numpy as np

from hip_util import KAT1_TOMATO, momentum_actions, scripted_then_random

EDGE_T = [1, 2, 255, 256, 257, 32767, 32768, 49999, 65535]
LIMITS = EDGE_T + [0]
N, STEPS, C, RADIUS, SEED = 101, 26, 3, 2, 41
LEVEL, BASE_LEVEL, BASE_AGENTS = "open-divider_tomato", "partial-divider_tl", 3
T_MAX = 0xFFFF
UNLIMITED_STARTS = [0, 1, 32767, 32768, 65533, 65534, 65535]

# KAT-1 (hip_util.KAT1_TOMATO) for the wrapper, whose players cannot stay: agent 0 walks to (4, 4) as
# in the script and then steps up and down between (4, 4) and (4, 3), off agent 1's way
# (column 1, row 5).  Checked on the CPU: it ends the episode by delivery on its 23rd step.
SOLVE = [(a0 if a0 < 4 else (1, 0)[(k - 5) % 2], a1) for k, (a0, a1) in enumerate(KAT1_TOMATO)]
SOLVING = 4                       # env i plays SOLVE from step 0 when i % SOLVING == 1


def start_list(T):
    """The start values of a time limit before cycling: 0, 1, T - 1 down to T - 8, T // 2, T // 3, and
    2^j - 1, 2^j for j = 7..15, clipped to [0, T - 1]; for T = 0 the fixed list around the field's
    edges."""
    if T == 0:
        return list(UNLIMITED_STARTS)
    raw = [0, 1] + [T - 1 - j for j in range(8)] + [T // 2, T // 3]
    for j in range(7, 16):
        raw += [2 ** j - 1, 2 ** j]
    return [min(max(v, 0), T - 1) for v in raw]


def start_values(T, n=N, index=None):
    """int32 [n]: env i starts at start_list(T)[i mod len] (`index`: the i of every env, default 0..n-1)."""
    lst = np.asarray(start_list(T), np.int64)
    idx = np.arange(n) if index is None else np.asarray(index)
    out = lst[idx % len(lst)].astype(np.int32)
    out.setflags(write=False)
    return out


def row0_with_t(row0, t):
    """State row 0 (int32 [n], numpy) with t in bits 16..31 and the low half as it is: int64
    arithmetic, then the two's-complement int32 (the word is negative from t = 32768 on)."""
    w = (np.asarray(row0).astype(np.int64) & 0xFFFF) | (np.asarray(t).astype(np.int64) << 16)
    return np.where(w >= 2 ** 31, w - 2 ** 32, w).astype(np.int32)


def inject_t(env, t):
    """Write t (int [n]) into bits 16..31 of env.state[0] on the device; the low 16 bits stay."""
    import torch
    t64 = torch.as_tensor(np.asarray(t).astype(np.int64), device=env.state.device)
    w = (env.state[0].to(torch.int64) & 0xFFFF) | (t64 << 16)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w)
    env.state[0].copy_(w.to(torch.int32))


@functools.lru_cache(maxsize=None)
def level(T, name=LEVEL, agents=2):
    from gym_comm_amd import compiler
    return compiler.compile_level(name, agents, T)


@functools.lru_cache(maxsize=None)
def fused_actions(n=N, steps=STEPS):
    """int32 [steps][4][n]: ego move, ego comm, alt move, alt comm (the ego is sim agent 0)."""
    rng = np.random.default_rng(SEED)
    mv = scripted_then_random(rng, LEVEL, steps, 2, n, nact=4)
    cm = rng.integers(0, C, (steps, 2, n))
    for i in range(1, n, SOLVING):
        for k in range(min(steps, len(SOLVE))):
            mv[k, 0, i], mv[k, 1, i] = SOLVE[k]
    acts = np.ascontiguousarray(np.stack([mv[:, 0], cm[:, 0], mv[:, 1], cm[:, 1]], axis=1).astype(np.int32))
    acts.setflags(write=False)
    return acts


@functools.lru_cache(maxsize=None)
def base_actions(n=N, steps=STEPS):
    """int32 [steps][3][n] NAV codes 0..4 (4 = stay); no solve script is known for this level."""
    acts = scripted_then_random(np.random.default_rng(SEED + 1), BASE_LEVEL, steps, BASE_AGENTS, n)
    acts = np.ascontiguousarray(acts.astype(np.int32))
    acts.setflags(write=False)
    return acts


def expected_t(t, done):
    """The kernels' counter after a step with auto-reset, as numbers: saturating at 65535, 0 where
    the episode ended."""
    return np.where(np.asarray(done) != 0, 0, np.minimum(np.asarray(t, np.int64) + 1, T_MAX)).astype(np.int32)


def _freeze(steps):
    for s in steps:
        for v in list(s.values()) + list(s["snapshot"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return steps


def run_fused(ora, acts, comm=None, radius=RADIUS):
    """Step an OracleBatch (already reset and set_t) through acts [K][4][n] with auto-reset: per step
    obs, timestep, reward, done, comm, the per-step metrics terms (OracleBatch.last_step), the
    snapshot, `reached` (the counter the step counted up to, before a possible reset: the oracle's,
    which does not saturate) and `timed_out` (done and not successful: env_done gives the limit
    precedence)."""
    n = ora.n
    comm = np.zeros((2, n), np.int32) if comm is None else comm
    steps = []
    t = ora.snapshot_all()["t"].astype(np.int64)
    for k in range(acts.shape[0]):
        o, ts, r, d = ora.multi_step(acts[k], comm, radius, 0, C, auto_reset=True)
        last = {key: v.copy() for key, v in ora.last_step().items()}
        snap = ora.snapshot_all()
        steps.append(dict(obs=o, timestep=ts, reward=r, done=d, comm=comm.copy(), snapshot=snap,
                          reached=t + 1, timed_out=((d != 0) & (last["success"] == 0)).astype(np.int32), **last))
        t = snap["t"].astype(np.int64)
    return steps


@functools.lru_cache(maxsize=None)
def fused_reference(T):
    """(t0 [N], the oracle's steps) of the fused input of time limit T."""
    from oracle import oracle
    oracle.build()
    t0 = start_values(T)
    ora = oracle.OracleBatch(level(T).blob, N)
    ora.set_t(t0)
    return t0, _freeze(run_fused(ora, fused_actions()))


@functools.lru_cache(maxsize=None)
def base_reference(T):
    """(t0 [N], the oracle's base steps) on BASE_LEVEL with three agents: per step reward, done,
    shaping, snapshot, reached and timed_out (the base step has no `successful` output: a done
    with reached < T, or any done at T = 0, is a delivery)."""
    from oracle import oracle
    oracle.build()
    t0 = start_values(T)
    acts = base_actions()
    ora = oracle.OracleBatch(level(T, BASE_LEVEL, BASE_AGENTS).blob, N)
    ora.set_t(t0)
    steps = []
    t = t0.astype(np.int64)
    for k in range(STEPS):
        r, d, sh = ora.step(acts[k], auto_reset=True)
        snap = ora.snapshot_all()
        timed = (d != 0) & (t + 1 >= T) & (T != 0)
        steps.append(dict(reward=r, done=d, shaping=sh, snapshot=snap, reached=t + 1, timed_out=timed.astype(np.int32)))
        t = snap["t"].astype(np.int64)
    return t0, _freeze(steps)


def table_row(t0, steps):
    """(envs that timed out at least once, the highest t a state row held): the two columns of the
    report, from a reference run.  What the device holds between launches is the start value and
    the counter after every step (0 after an auto-reset, 65535 at most)."""
    timed = np.zeros(len(t0), bool)
    top = int(np.max(t0))
    for s in steps:
        timed |= s["timed_out"] != 0
        top = max(top, int(np.minimum(s["snapshot"]["t"], T_MAX).max()))
    return int(timed.sum()), top


# ---- the map set with a time limit per map ---------------------------------------------------------
SET_MAPS = ("open-divider_tomato", "partial-divider_tomato", "full-divider_tomato")
SET_T = (1, 32768, 65535)
SET_GROUPS = (0, 1, 2, 2)
SET_N = 3 * 64 + 37


def set_env_map():
    return np.asarray(SET_GROUPS)[np.arange(SET_N) // 64]


def set_levels():
    import mapset_inputs as mi
    return [mi.compiled(m, T) for m, T in zip(SET_MAPS, SET_T)]


def set_start_values():
    """int32 [SET_N]: env i starts at its own map's start_values, indexed by its place in the batch."""
    em = set_env_map()
    out = np.zeros(SET_N, np.int32)
    for m, T in enumerate(SET_T):
        ix = np.nonzero(em == m)[0]
        out[ix] = start_values(T, index=ix)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def set_reference():
    """(t0, steps) of the map set under one oracle per map (test_mapset_gpu.SetOracle, which steps
    with that module's C = 3 and radius 2: the values used here)."""
    from oracle import oracle
    from test_mapset_gpu import SetOracle
    oracle.build()
    t0 = set_start_values()
    acts = fused_actions(SET_N)
    ora = SetOracle(set_levels(), SET_GROUPS, SET_N)
    ora.reset()
    for m, o, ix in ora._each():
        o.set_t(np.ascontiguousarray(t0[ix]))
    steps = [ora.multi_step(acts[k]) for k in range(STEPS)]
    return t0, _freeze(steps)


# ---- the quotient sweep ------------------------------------------------------------------------------
def sweep_limits():
    """The edge limits plus 24 seeded ones from 3..65534."""
    extra = np.random.default_rng(SEED + 2).choice(np.arange(3, 65535), size=24, replace=False)
    return EDGE_T + sorted(int(v) for v in extra)
