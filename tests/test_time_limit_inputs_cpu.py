"""No GPU: what test_time_limit_gpu.py relies on, checked with the oracle alone.

  ``set_t`` (oracle/oc_oracle.c: oc_oracle_debug_set_t) is not trusted: an episode started at t = k
    equals one that made k all-stay steps, output by output, for the base step and the wrapper step;
  the inputs of tests/time_limit_inputs.py reach what the GPU cases are about -- envs that time out
    inside the window, envs that go on counting from 0 behind a reset, envs that never time out,
    a counter with bit 15 set, an episode that ends by delivery -- and raise no flag;
  the word written into state row 0 keeps the low half and goes negative from 32768;
  the host refuses a time limit outside the 16-bit field.
"""
import numpy as np
import pytest

import time_limit_inputs as tl
from hip_util import bits, momentum_actions

T_SET, TAPE = 257, 12
KS = [0, 1, 250, 300]
NB = 8                          # envs per oracle batch: every env plays its own column of the tape


def _same(a, b):
    for key in ("items", "order", "agents", "t", "nobj", "completed", "goal_count", "error"):
        assert np.array_equal(a[key], b[key]), key


def _batch(name, agents):
    from oracle import oracle
    oracle.build()
    ora = oracle.OracleBatch(tl.level(T_SET, name, agents).blob, NB)
    ora.reset()
    return ora


def test_an_all_stay_step_changes_nothing_but_t():
    stay = np.full((tl.BASE_AGENTS, NB), 4, np.int32)
    ora = _batch(tl.BASE_LEVEL, tl.BASE_AGENTS)
    before = ora.snapshot_all()
    r, d, sh = ora.step(stay)
    after = ora.snapshot_all()
    assert (after["t"] == before["t"] + 1).all() and not r.any() and not d.any()
    _same(dict(before, t=before["t"] + 1), after)
    # the wrapper: nobody CAN_MOVE, so both players stand (overcooked_env.py:250-262)
    ora = _batch(tl.LEVEL, 2)
    before = ora.snapshot_all()
    comm = np.zeros((2, NB), np.int32)
    ora.multi_step(np.zeros((4, NB), np.int32), comm, tl.RADIUS, 0, tl.C, can_move_mask=0)
    after = ora.snapshot_all()
    _same(dict(before, t=before["t"] + 1), after)


@pytest.mark.parametrize("k", KS)
def test_set_t_equals_k_all_stay_steps_base(k):
    """Oracle A makes k all-stay steps (no auto-reset: at k = 300 the counter walks past T = 257 and
    stays there), oracle B is set to t = k; both then play one seeded tape of 12 steps with auto-reset.
    k = 250 crosses the limit on the tape's seventh step, k = 300 on its first."""
    tape = momentum_actions(np.random.default_rng(100 + k), TAPE, tl.BASE_AGENTS, NB)
    a, b = _batch(tl.BASE_LEVEL, tl.BASE_AGENTS), _batch(tl.BASE_LEVEL, tl.BASE_AGENTS)
    stay = np.full((tl.BASE_AGENTS, NB), 4, np.int32)
    for _ in range(k):
        a.step(stay, auto_reset=False)
    b.set_t(np.full(NB, k, np.int32))
    _same(a.snapshot_all(), b.snapshot_all())
    assert (b.snapshot_all()["t"] == k).all()
    dones = 0
    for j in range(TAPE):
        ra, da, sa = a.step(tape[j], auto_reset=True)
        rb, db, sb = b.step(tape[j], auto_reset=True)
        assert np.array_equal(ra, rb) and np.array_equal(da, db) and np.array_equal(bits(sa), bits(sb)), j
        _same(a.snapshot_all(), b.snapshot_all())
        dones += int(da.sum())
    assert dones == (NB if k >= 250 else 0)
    assert not a.snapshot_all()["error"].any()


@pytest.mark.parametrize("k", KS)
def test_set_t_equals_k_all_stay_steps_wrapper(k):
    """The same through OvercookedMultiEnv.multi_step: both viewers' rows, the timestep bits, the
    shaped reward, done and the comm rows of every tape step, and the final snapshots."""
    rng = np.random.default_rng(200 + k)
    tape = np.stack([rng.integers(0, 4, (TAPE, NB)), rng.integers(0, tl.C, (TAPE, NB)),
                     rng.integers(0, 4, (TAPE, NB)), rng.integers(0, tl.C, (TAPE, NB))], axis=1).astype(np.int32)
    a, b = _batch(tl.LEVEL, 2), _batch(tl.LEVEL, 2)
    ca, cb = np.zeros((2, NB), np.int32), np.zeros((2, NB), np.int32)
    idle = np.zeros((4, NB), np.int32)
    for _ in range(k):
        a.multi_step(idle, ca, tl.RADIUS, 0, tl.C, can_move_mask=0, auto_reset=False)
    cb[:] = ca                   # (the comm rows belong to the caller, not to the env)
    b.set_t(np.full(NB, k, np.int32))
    _same(a.snapshot_all(), b.snapshot_all())
    for j in range(TAPE):
        oa, ta, ra, da = a.multi_step(tape[j], ca, tl.RADIUS, 0, tl.C, auto_reset=True)
        ob, tb, rb, db = b.multi_step(tape[j], cb, tl.RADIUS, 0, tl.C, auto_reset=True)
        assert np.array_equal(oa, ob) and np.array_equal(bits(ta), bits(tb)), j
        assert np.array_equal(bits(ra), bits(rb)) and np.array_equal(da, db) and np.array_equal(ca, cb), j
        want = (a.snapshot_all()["t"]).astype(np.float64) / T_SET
        assert np.array_equal(bits(ta), bits(want)), j
    _same(a.snapshot_all(), b.snapshot_all())


def test_single_env_set_t():
    from oracle import oracle
    oracle.build()
    e = oracle.OracleEnv(tl.level(T_SET).blob)
    e.reset()
    before = e.snapshot()
    e.set_t(40000)
    after = e.snapshot()
    assert after["t"] == 40000
    _same(dict(before, t=40000, error=0), dict(after, error=0))
    assert e.obs(0, tl.RADIUS, False, False, tl.C, [0, 0])[1] == 40000 / T_SET


# ---- the inputs ----------------------------------------------------------------------------------
def test_start_values_and_the_injected_word():
    for T in tl.EDGE_T:
        lst = tl.start_list(T)
        assert len(lst) == 30 and min(lst) >= 0 and max(lst) <= T - 1
        t0 = tl.start_values(T)
        assert t0.shape == (tl.N,) and t0.dtype == np.int32 and t0[0] == 0 and t0[31] == min(1, T - 1)
    assert tl.start_list(65535)[:12] == [0, 1, 65534, 65533, 65532, 65531, 65530, 65529, 65528, 65527, 32767, 21845]
    assert tl.start_list(65535)[12:16] == [127, 128, 255, 256] and tl.start_list(65535)[-2:] == [32767, 32768]
    assert tl.start_list(255)[14] == 254 and sorted(set(tl.start_values(0).tolist())) == tl.UNLIMITED_STARTS
    assert tl.N == 64 + 37 and tl.SET_N == 3 * 64 + 37
    # the word: the low half stays, the sign bit is t's bit 15
    low = np.array([0x0321, 0x0F45, 0xFFFF, 0x0012], np.int32)
    w = tl.row0_with_t(low, [1, 32767, 32768, 65535])
    assert w.dtype == np.int32 and w.tolist() == [0x10321, 0x7FFF0F45, -0x80000000 + 0xFFFF, -0x10000 + 0x12]
    assert ((w.astype(np.int64) >> 16) & 0xFFFF).tolist() == [1, 32767, 32768, 65535]
    assert ((w & 0xFFFF) == low).all()
    # the sweep's limits: the edges and 24 distinct others, the same every time
    sw = tl.sweep_limits()
    assert sw[:9] == tl.EDGE_T and len(set(sw)) == 33 and all(3 <= v <= 65534 for v in sw[9:])
    assert sw == tl.sweep_limits()


def test_the_solve_script_without_a_stay_delivers_on_its_last_step():
    from oracle import oracle
    oracle.build()
    assert len(tl.SOLVE) == 23 and all(0 <= a < 4 and 0 <= b < 4 for a, b in tl.SOLVE)
    ora = oracle.OracleBatch(tl.level(0).blob, 1)
    comm = np.zeros((2, 1), np.int32)
    for k, (a0, a1) in enumerate(tl.SOLVE):
        _, _, _, d = ora.multi_step(np.array([[a0], [0], [a1], [0]], np.int32), comm, tl.RADIUS, 0, tl.C)
        assert int(d[0]) == (k == 22), k
    assert int(ora.last_step()["success"][0]) == 1


def _conditions(T, t0, steps):
    n = len(t0)
    assert len(steps) == tl.STEPS
    assert all(int((s["snapshot"]["error"] != 0).sum()) == 0 for s in steps), "an env-step was flagged"
    timed = np.stack([s["timed_out"] for s in steps])               # [STEPS][n]
    done = np.stack([s["done"] for s in steps])
    reached = np.stack([s["reached"] for s in steps])
    after = np.stack([s["snapshot"]["t"] for s in steps])
    per_env = timed.sum(axis=0)
    if T == 0:
        assert per_env.sum() == 0
        return dict(timed_out=0, delivered=int(done.sum()))
    assert (timed == ((reached >= T) & (done != 0))).all() and (reached <= T).all()
    if T <= 2:
        assert per_env.min() >= 5, per_env.min()
        return dict(timed_out=int((per_env > 0).sum()))
    # behind its first time-out an env goes on counting from 0
    first = np.where(per_env > 0, timed.argmax(axis=0), tl.STEPS)
    crossed = [i for i in range(n) if first[i] < tl.STEPS - 1 and after[first[i], i] == 0 and after[first[i] + 1, i] == 1]
    assert int((per_env > 0).sum()) >= 8, "timed out"
    assert len(crossed) >= 8, "crossed a reset"
    assert int((per_env == 0).sum()) >= 20, "never timed out"
    if T >= 32768:
        assert (reached >= 32768).any()
    return dict(timed_out=int((per_env > 0).sum()), crossed=len(crossed), never=int((per_env == 0).sum()),
                delivered=int(((done != 0) & (timed == 0)).sum()))


@pytest.mark.parametrize("T", tl.LIMITS)
def test_fused_inputs_reach_what_the_gpu_cases_need(T):
    """Every condition under the oracle alone; done by delivery (successful, not timed out) happens
    in every case with T >= 255 and at T = 0.  A counter of 32768 and more is `reached`, the value
    a step counts up to: at T = 32768 it exists only inside the step that times out, at T = 49999
    and 65535 (and 0) the state itself holds such values between steps."""
    t0, steps = tl.fused_reference(T)
    got = _conditions(T, t0, steps)
    if T == 0 or T >= 255:
        success = sum(int((s["success"] != 0).sum()) for s in steps)
        assert success >= 1 and got["delivered"] == success
    if T == 0:
        assert max(int(s["snapshot"]["t"].max()) for s in steps) > tl.T_MAX     # the oracle counts past the field
    if T in (49999, 65535):
        assert max(int(s["snapshot"]["t"].max()) for s in steps) >= 32768
    envs, top = tl.table_row(t0, steps)
    assert envs == got["timed_out"] and top == (tl.T_MAX if T == 0 else T - 1)


@pytest.mark.parametrize("T", tl.LIMITS)
def test_base_inputs_reach_what_the_gpu_cases_need(T):
    """The three-agent base step's input meets the conditions on the counter.  No episode of
    partial-divider_tl ends by delivery inside the window (two deliveries, no known script): the
    delivery condition is the fused input's."""
    t0, steps = tl.base_reference(T)
    _conditions(T, t0, steps)


def test_map_set_inputs_time_out_per_map():
    """T = (1, 32768, 65535) on three maps: map 0's envs time out on every step, the others at their
    own limit only; every map's start values come from its own list."""
    t0, steps = tl.set_reference()
    em = tl.set_env_map()
    assert np.bincount(em).tolist() == [64, 64, 101]
    done = np.stack([s["done"] for s in steps])
    assert (done[:, em == 0] == 1).all()
    for m in (1, 2):
        T = tl.SET_T[m]
        col = np.nonzero(em == m)[0]
        assert (t0[col] <= T - 1).all() and (t0[col] == T - 1).any()
        ends = done[:, col].sum(axis=0)
        assert (ends > 0).sum() >= 8 and (ends == 0).sum() >= 20
    assert all(int((s["snapshot"]["error"] != 0).sum()) == 0 for s in steps)
    # the timestep is t over the env's own limit
    Ts = np.asarray(tl.SET_T, np.float64)[em]
    for s in steps:
        assert np.array_equal(bits(s["timestep"]), bits(s["snapshot"]["t"].astype(np.float64) / Ts))


# ---- the host's refusals -------------------------------------------------------------------------
T_WORD = 7                      # include/oc_level.h: OC_LV_T


@pytest.mark.parametrize("T", [65536, -1, 1 << 20])
def test_a_time_limit_outside_the_field_is_refused(T):
    from gym_comm_amd import _lib, specialize
    blob = tl.level(100).blob.copy()
    assert blob[T_WORD] == 100
    blob[T_WORD] = T
    for geometry in (True, False):
        with pytest.raises(_lib.OcError, match="level dimensions out of range"):
            specialize.spec_header_text(blob, geometry)
    with pytest.raises(_lib.OcError, match="level dimensions out of range"):
        _lib.subtask_info(blob)


@pytest.mark.parametrize("T", [65535, 0])
def test_the_fields_ends_are_accepted(T):
    from gym_comm_amd import _lib, specialize
    blob = tl.level(T).blob
    assert blob[T_WORD] == T
    assert specialize.spec_header_text(blob, True) == specialize.spec_header_text(tl.level(100).blob, True)
    _lib.subtask_info(blob)
